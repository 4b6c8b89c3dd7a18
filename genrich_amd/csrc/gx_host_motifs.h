// gx_host_motifs.h -- the host side of the sequence and the motif scan (gx_motifs.h): the third vector's switch, the letters
// read back, the motifs' tables with both strands packed, the regions resolved to units, the pass with its counted list (run
// once more when it ran full), the sorted hits; the pass over a caller's regions, over the called peaks and over the genome.
// (a part of gx_api.hip's translation unit)
#pragma once
namespace {

static_assert(sizeof(MotHit) == sizeof(gx_motif_hit) && sizeof(gx_motif_hit) == 16 && offsetof(MotHit, score) == offsetof(gx_motif_hit, score) &&
              offsetof(MotHit, motif) == offsetof(gx_motif_hit, motif) && offsetof(MotHit, strand) == offsetof(gx_motif_hit, strand), "MotHit is gx_motif_hit");
static_assert(MOT_MAX_WIDTH == GX_MOTIF_MAX_WIDTH && MOT_MAX == GX_MOTIF_MAX, "the header's limits are the kernel's");

// gx_set_genome_bases: the third vector appears (cleared, with the other two) or goes
int seq_set_bases(gx_ctx* ctx, bool on) {
  if (!ctx->gcOn) return refuse(ctx, "gx_set_genome_bases comes after gx_set_genome(ctx, 1)");
  if (on == ctx->seqOn) return GX_OK;
  if (!on) {
    ctx->seqOn = false;
    ctx->gcAg.release();
    return GX_OK;
  }
  if (!ctx->gcDirty)
    for (uint64_t p : ctx->gcPushed)
      if (p) return refuse(ctx, "gx_set_genome_bases comes before the first base is pushed (gx_push_sequence)");
  ctx->seqOn = true;
  if (int rc = gc_layout(ctx)) {
    ctx->seqOn = false;
    return rc;
  }
  return GX_OK;
}

// gx_get_sequence: n letters of a chromosome from `start` on
int seq_get(gx_ctx* ctx, int chrom, uint64_t start, size_t n, char* out) {
  if (!ctx->seqOn) return refuse(ctx, "gx_get_sequence needs the bases (gx_set_genome_bases)");
  if (int rc = gc_current(ctx)) return rc;
  if (chrom < 0 || (u32)chrom >= ctx->nChrom) return refuse(ctx, "gx_get_sequence: a chromosome outside the table");
  if ((u64)n >> 32 || start >> 32) return refuse(ctx, "gx_get_sequence: 2^32 bases or more");
  if (!n) return GX_OK;
  const GcChrom cc = ctx->gcChrom[chrom];
  const u64 n4 = ((u64)n + 3) / 4;
  hipStream_t s = ctx->stream;
  POOLED(ctx, ctx->seqOut, (size_t)n4 * 4);
  phase_begin(ctx, "seq.unpack");
  hipLaunchKernelGGL(k_seq_unpack, dim3((unsigned)((n4 + MOT_NT - 1) / MOT_NT)), dim3(MOT_NT), 0, s, ctx->gcVec.as<unsigned long long>(),
                     ctx->gcAg.as<unsigned long long>(), ctx->gcAcgt.as<unsigned long long>(), cc.off, cc.len, cc.laid, (u64)start, n4, ctx->seqOut.as<u32>());
  if (int rc__ = dbg_sync(ctx, "k_seq_unpack")) return rc__;
  HIPCHECK(hipGetLastError());
  phase_end(ctx);
  HIPCHECK(hipMemcpyAsync(out, ctx->seqOut.p, n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  ctx->gcUsed = true;
  return GX_OK;
}

// gx_set_motifs: the limits, then each motif's table in raw-code order with the reverse strand in the high halves
int mot_set(gx_ctx* ctx, const gx_motif* m, int n, const int16_t* scores) {
  if (n < 0 || n > (int)MOT_MAX) return refuse(ctx, "gx_set_motifs: more than 4096 motifs");
  for (int i = 0; i < n; i++)
    if (m[i].width < 1 || m[i].width > MOT_MAX_WIDTH) return refuse(ctx, "gx_set_motifs: a motif's width must satisfy 1 <= L <= 32");
  static const u32 columnOf[4] = {3, 0, 1, 2};   // raw code T A C G -> its column in A C G T
  ctx->motMeta.assign((size_t)n, MotMeta{0, 0});
  ctx->motTabs.assign((size_t)n * MOT_TAB_WORDS, 0);
  for (int i = 0; i < n; i++) {
    const u32 L = m[i].width;
    const int16_t* s = scores + m[i].offset;
    ctx->motMeta[i] = MotMeta{L, m[i].threshold};
    for (u32 j = 0; j < L; j++)
      for (u32 r = 0; r < 4; r++) {
        const int f = s[4 * j + columnOf[r]], v = s[4 * (L - 1 - j) + columnOf[r ^ 1u]];
        ctx->motTabs[(size_t)i * MOT_TAB_WORDS + 4 * j + r] = (int)(((u32)v << 16) | ((u32)f & 0xffffu));
      }
  }
  ctx->motDirty = true;
  ctx->motReady = false;
  ctx->motHits.clear();
  ctx->motCounts.clear();
  return GX_OK;
}

struct MotGeometry { unsigned grid; u32 step, batch; u64 listCap; };

// the geometry's refusals and the grid of a pass over nUnits units (gx_motif_grid; no device): a workgroup's MOT_NW wavefronts
// add to the same 32-bit LDS counters, at most 64 per run, so a workgroup walks at most MOT_FLUSH_RUNS runs per batch
int mot_grid(u64 nUnits, u32 step, unsigned grid, unsigned* chosen, const char** why) {
  if (step < 1 || step > MOT_MAX_STEP) return *why = "motifs: a step must be 1 to 16 words", GX_ERR_ORDER;
  if (grid > MOT_MAX_GRID) return *why = "motifs: more than 65535 workgroups", GX_ERR_ORDER;
  if (nUnits >> 32) return *why = "motifs: 2^32 units of positions or more", GX_ERR_ORDER;
  const u64 need = mot_need_grid(nUnits, step);
  if (grid && grid < need) return *why = "motifs: a grid that lets a workgroup walk more than 2^25 runs (its 32-bit counters)", GX_ERR_ORDER;
  *chosen = grid ? grid : (unsigned)std::max<u64>(std::max<u64>(need, 1), std::min<u64>((nUnits + MOT_NW - 1) / MOT_NW, MOT_GRID));
  return GX_OK;
}

// The regions that have a position at all (on a chromosome of the table that is laid out, clamped to its length) as MotRegion
// records with the units before each; the units of all (2^32 or more: the caller's mot_grid refuses), their positions added to
// *positions.  Shared with the k-mer pass (gx_host_kmers.h).
u64 mot_resolve(const gx_ctx* ctx, const gx_region* reg, size_t n, u32 step, std::vector<MotRegion>& rs, u64* positions) {
  u64 nUnits = 0;
  for (size_t i = 0; i < n && !(nUnits >> 32); i++) {
    if (reg[i].chrom >= ctx->nChrom) continue;
    const GcChrom& cc = ctx->gcChrom[reg[i].chrom];
    const u32 e = std::min(reg[i].end, cc.len);
    if (!cc.laid || reg[i].start >= e) continue;
    rs.push_back(MotRegion{cc.off, reg[i].start, e, (u32)i, (u32)nUnits});
    *positions += e - reg[i].start;
    const u64 runs = ((u64)(e - reg[i].start) + 63) / 64;
    nUnits += (runs + step - 1) / step;
  }
  return nUnits;
}

// a pass that is set up: its arguments, its grid, what must live until the stream is drained
struct MotRun {
  MotArgs a{};
  unsigned grid = 0;
  size_t lds = 0, words = 0;
  u64 positions = 0;                       // of all regions
  std::vector<MotRegion> rs;
  std::vector<unsigned long long> h;       // the control words and counts, read back
  bool live = false;                       // there is something to launch
};

// the refusals, the regions that have a position at all with their units, the grid, the motifs and the regions on the device
int mot_setup(gx_ctx* ctx, const gx_region* reg, size_t n, MotGeometry g, MotRun& r) {
  const u32 nM = (u32)ctx->motMeta.size();
  ctx->motLastReruns = ctx->motLastBatches = 0;
  if (g.step == 0) g.step = MOT_STEP;
  if (g.batch == 0) g.batch = MOT_BATCH;
  if (g.batch > MOT_BATCH) return refuse(ctx, "motifs: a batch must be 1 to 64 motifs");
  if (g.listCap >= MOT_MAX_HITS) return refuse(ctx, "motifs: a hit list of 2^31 entries or more");
  if (n >> 32) return refuse(ctx, "motifs: 2^32 regions or more");
  const char* why = "";
  if (mot_grid(0, g.step, g.grid, &r.grid, &why)) return refuse(ctx, why);   // (the step and the grid, before anything is done)
  if (int rc = gc_current(ctx)) return rc;
  const u64 nUnits = mot_resolve(ctx, reg, n, g.step, r.rs, &r.positions);
  if (mot_grid(nUnits, g.step, g.grid, &r.grid, &why)) return refuse(ctx, why);
  if (!nM || r.rs.empty()) return GX_OK;
  hipStream_t s = ctx->stream;
  if (ctx->motDirty) {
    POOLED(ctx, ctx->motTabDev, ctx->motTabs.size() * 4);
    POOLED(ctx, ctx->motMetaDev, ctx->motMeta.size() * sizeof(MotMeta));
    HIPCHECK(hipMemcpyAsync(ctx->motTabDev.p, ctx->motTabs.data(), ctx->motTabs.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->motMetaDev.p, ctx->motMeta.data(), ctx->motMeta.size() * sizeof(MotMeta), hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));
    ctx->motDirty = false;
  }
  r.words = MOC_WORDS + (size_t)3 * nM;
  r.h.assign(r.words, 0);
  POOLED(ctx, ctx->motReg, r.rs.size() * sizeof(MotRegion));
  POOLED(ctx, ctx->motOut, r.words * 8);
  HIPCHECK(hipMemcpyAsync(ctx->motReg.p, r.rs.data(), r.rs.size() * sizeof(MotRegion), hipMemcpyHostToDevice, s));
  MotArgs& a = r.a;
  a.gc = ctx->gcVec.as<unsigned long long>();
  a.ag = ctx->gcAg.as<unsigned long long>();
  a.acgt = ctx->gcAcgt.as<unsigned long long>();
  a.reg = ctx->motReg.as<MotRegion>();
  a.nReg = (u32)r.rs.size();
  a.nUnits = (u32)nUnits;
  a.step = g.step;
  a.tabs = ctx->motTabDev.as<int>();
  a.meta = ctx->motMetaDev.as<MotMeta>();
  a.nMotif = nM;
  a.batch = std::min(g.batch, nM);
  a.out = ctx->motOut.as<unsigned long long>();
  r.lds = mot_lds_bytes(a.batch);
  r.live = true;
  return GX_OK;
}

// the counts [3][nMotif] (windows, hits +, hits -) of a pass whose words are in r.h; *total: its hits
void mot_counts(gx_ctx* ctx, const MotRun& r, std::vector<uint64_t>& counts, u64* total) {
  const u32 nM = (u32)ctx->motMeta.size();
  counts.assign((size_t)3 * nM, 0);
  *total = 0;
  if (!r.live) return;
  ctx->motUsed = true;
  ctx->motLastBatches = (nM + r.a.batch - 1) / r.a.batch;
  for (u32 m = 0; m < nM; m++)
    for (u32 k = 0; k < 3; k++) {
      counts[(size_t)k * nM + m] = r.h[MOC_WORDS + 3 * (size_t)m + k];
      if (k) *total += counts[(size_t)k * nM + m];
    }
}

// The count-only pass in two halves, so that several contexts' passes run side by side: launched with its read-back queued ...
int mot_count_begin(gx_ctx* ctx, const gx_region* reg, size_t n, MotRun& r) {
  if (int rc = mot_setup(ctx, reg, n, MotGeometry{0, 0, 0, 0}, r)) return rc;
  if (!r.live) return GX_OK;
  hipStream_t s = ctx->stream;
  phase_begin(ctx, "motifs");
  HIPCHECK(hipMemsetAsync(ctx->motOut.p, 0, r.words * 8, s));
  hipLaunchKernelGGL(k_motif_scan<false>, dim3(r.grid), dim3(MOT_NT), r.lds, s, r.a);
  if (int rc__ = dbg_sync(ctx, "k_motif_scan<count>")) return rc__;
  HIPCHECK(hipGetLastError());
  phase_end(ctx);
  HIPCHECK(ctx->motHost.ensure(r.words * 8));   // (pinned: the copy is queued, the host goes on to the next context)
  HIPCHECK(hipMemcpyAsync(ctx->motHost.p, ctx->motOut.p, r.words * 8, hipMemcpyDeviceToHost, s));
  return GX_OK;
}
// ... and drained
int mot_count_end(gx_ctx* ctx, MotRun& r, std::vector<uint64_t>& counts) {
  if (r.live) {
    HIPCHECK(hipStreamSynchronize(ctx->stream));   // (the regions' host copy may go)
    memcpy(r.h.data(), ctx->motHost.p, r.words * 8);
  }
  u64 total = 0;
  mot_counts(ctx, r, counts, &total);
  return GX_OK;
}

// One pass over reg[n] with the hit list: the counts and the sorted hits.  g: 0 means the library's choice.
int mot_pass(gx_ctx* ctx, const gx_region* reg, size_t n, MotGeometry g, std::vector<gx_motif_hit>& hits, std::vector<uint64_t>& counts) {
  hits.clear();
  MotRun r;
  if (int rc = mot_setup(ctx, reg, n, g, r)) return rc;
  u64 total = 0;
  if (!r.live) return mot_counts(ctx, r, counts, &total), GX_OK;
  hipStream_t s = ctx->stream;
  // the first list: the caller's, else room for one hit in MOT_LIST_SHARE windows of every motif on both strands (p = 1e-4 needs
  // a fifth of it), between the least and the most a first list takes
  const u64 guess = std::min<u64>(std::max<u64>(MOT_LIST_MIN, r.positions / MOT_LIST_SHARE * r.a.nMotif), MOT_LIST_FIRST_MAX);
  phase_begin(ctx, "motifs");
  CountedList list{"motifs", "hit list", &ctx->motList, sizeof(MotHit), &ctx->motOut, r.words, MOC_STATUS, MOC_COUNT, MOT_ST_LIST_FULL,
                   0, "", g.listCap ? g.listCap : guess};
  if (int rc = counted_list(ctx, list, r.h, [&](u32 cap) -> int {
        if (cap >= MOT_MAX_HITS) return refuse(ctx, "motifs: 2^31 hits or more");
        r.a.list = ctx->motList.as<MotHit>();
        r.a.listCap = cap;
        hipLaunchKernelGGL(k_motif_scan<true>, dim3(r.grid), dim3(MOT_NT), r.lds, s, r.a);
        if (int rc__ = dbg_sync(ctx, "k_motif_scan")) return rc__;
        HIPCHECK(hipGetLastError());
        return GX_OK;
      }))
    return rc;
  phase_end(ctx);
  ctx->motLastReruns = list.reruns;
  mot_counts(ctx, r, counts, &total);
  if (r.h[MOC_COUNT] != total) {
    ctx->err = "motifs: the hit list does not have the hits counted (a lost or doubled contribution)";
    return GX_ERR_DEVICE;
  }
  hits.resize((size_t)total);
  if (total) {
    HIPCHECK(hipMemcpyAsync(hits.data(), ctx->motList.p, (size_t)total * sizeof(MotHit), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
  // the records come in the order of the races
  std::sort(hits.begin(), hits.end(), gx_peak_merge::by_peak(&gx_motif_hit::region, gx_peak_merge::motif_hit_less));
  return GX_OK;
}

// min(cap, motifs) of each count to the caller
int mot_give(const std::vector<uint64_t>& counts, size_t nM, uint64_t* windows, uint64_t* hitsF, uint64_t* hitsR, size_t cap) {
  const size_t k = std::min(cap, nM);
  if (k && (!windows || !hitsF || !hitsR)) return GX_ERR_ORDER;
  if (k) {
    std::copy(counts.begin(), counts.begin() + k, windows);
    std::copy(counts.begin() + nM, counts.begin() + nM + k, hitsF);
    std::copy(counts.begin() + 2 * nM, counts.begin() + 2 * nM + k, hitsR);
  }
  return GX_OK;
}

// the peaks gx_find_peaks left on this context
int mot_scan_peaks(gx_ctx* ctx) {
  const size_t nPk = ctx->nHostPeaks;
  const gx_peak* hp = static_cast<const gx_peak*>(ctx->hPeaks.p);
  std::vector<gx_region> reg(nPk);
  for (size_t k = 0; k < nPk; k++) reg[k] = gx_region{hp[k].chrom, hp[k].start, hp[k].end};
  ctx->motReady = false;
  if (int rc = mot_pass(ctx, reg.data(), nPk, MotGeometry{0, 0, 0, 0}, ctx->motHits, ctx->motCounts)) return rc;
  ctx->motReady = true;
  return GX_OK;
}

// every chromosome that takes part: laid out (not skipped, owned) and saved
std::vector<gx_region> mot_genome_regions(const gx_ctx* ctx) {
  std::vector<gx_region> reg;
  for (u32 c = 0; c < ctx->nChrom; c++)
    if (ctx->gcChrom[c].laid && ctx->save[c]) reg.push_back(gx_region{c, 0, ctx->gcChrom[c].len});
  return reg;
}

void drop_motifs(gx_ctx* ctx) {   // gx_reset: the results go, the motifs and the genome stay
  ctx->motHits.clear();
  ctx->motCounts.clear();
  ctx->motReady = ctx->motUsed = false;
}

}  // namespace
