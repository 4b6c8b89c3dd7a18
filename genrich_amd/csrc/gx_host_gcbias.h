// gx_host_gcbias.h -- the host side of the reference sequence and the GC figures (gx_gcbias.h): the layout of the two bit
// vectors with their padding, the bases' way to the device (gx_push_sequence), the rank directory behind its dirty flag, the
// content of given intervals, the expected table per set of chromosomes, the observed tables per view, the pass over the kept
// samples and the one over a caller's events, the sum over contexts.  (a part of gx_api.hip's translation unit)
#pragma once
#include <map>
namespace {

constexpr size_t GC_PUSH = (size_t)1 << 24;   // bases per pinned staging buffer (16 MiB) and per k_gc_pack launch of gx_push_sequence

bool gc_chrom_laid_out(const gx_ctx* ctx, u32 c) { return !ctx->skip[c] && ctx->owned[c] && ctx->len[c] != 0; }
u64 gc_round_block(u64 w) { return (w + GC_BLOCK_WORDS - 1) / GC_BLOCK_WORDS * GC_BLOCK_WORDS; }
// the words allocated for vectors of `words` words: a tile of k_gc_expected reads its span beyond the last chromosome
u64 gc_alloc_words(u64 words) { return gc_round_block(words + GC_MAX_TILE + GC_PAD + 2); }

int gc_check_window(gx_ctx* ctx, int window) {
  if (window < 1 || window > (int)GC_MAX_WINDOW) return refuse(ctx, "GC bias: the window must satisfy 1 <= W <= 4096");
  return GX_OK;
}

// the vectors for the context's table, empty (after gx_set_genome, and again when gx_set_chroms / gx_set_owned changed the table)
int gc_layout(gx_ctx* ctx) {
  u64 bits = 0;
  for (u32 c = 0; c < ctx->nChrom; c++)
    if (gc_chrom_laid_out(ctx, c)) bits += ctx->len[c];
  if (bits >= GC_MAX_BITS) return refuse(ctx, "genome: 2^37 bases or more");
  ctx->gcChrom.assign(ctx->nChrom, GcChrom{0, 0, 0});
  u64 at = gc_round_block(GC_PAD);
  for (u32 c = 0; c < ctx->nChrom; c++) {
    ctx->gcChrom[c].len = ctx->len[c];
    if (!gc_chrom_laid_out(ctx, c)) continue;
    ctx->gcChrom[c].off = at;
    ctx->gcChrom[c].laid = 1;
    at = gc_round_block(at + ((u64)ctx->len[c] + 63) / 64 + GC_PAD);
  }
  ctx->gcWords = at;
  const size_t bytes = (size_t)gc_alloc_words(at) * 8;
  if (ctx->gcVec.ensure(bytes) != hipSuccess || ctx->gcAcgt.ensure(bytes) != hipSuccess || ctx->gcDir.ensure(bytes / GC_BLOCK_WORDS) != hipSuccess ||
      ctx->gcTab.ensure((size_t)ctx->nChrom * sizeof(GcChrom)) != hipSuccess)
    return pool_failed(ctx);
  hipStream_t s = ctx->stream;
  if (ctx->seqOn) {   // (gx_set_genome_bases: the third vector, with the other two)
    if (ctx->gcAg.ensure(bytes) != hipSuccess) return pool_failed(ctx);
    HIPCHECK(hipMemsetAsync(ctx->gcAg.p, 0, bytes, s));
  }
  HIPCHECK(hipMemsetAsync(ctx->gcVec.p, 0, bytes, s));
  HIPCHECK(hipMemsetAsync(ctx->gcAcgt.p, 0, bytes, s));
  HIPCHECK(hipMemcpyAsync(ctx->gcTab.p, ctx->gcChrom.data(), (size_t)ctx->nChrom * sizeof(GcChrom), hipMemcpyHostToDevice, s));
  HIPCHECK(hipStreamSynchronize(s));
  ctx->gcPushed.assign(ctx->nChrom, 0);
  ctx->gcDirty = false;
  ctx->gcDirDirty = true;
  return GX_OK;
}

void drop_gcbias(gx_ctx* ctx) {   // gx_reset: the results go, the genome stays
  ctx->gcRes.clear();
  ctx->gcReady = ctx->gcUsed = false;
}

int gc_current(gx_ctx* ctx) { return ctx->gcDirty ? gc_layout(ctx) : GX_OK; }

// gx_push_sequence: through two pinned staging buffers to one device buffer and k_gc_pack, all on the context's stream (the
// caller's memory is free on return)
int gc_push(gx_ctx* ctx, int chrom, uint64_t first, const char* bases, size_t n) {
  if (int rc = gc_current(ctx)) return rc;
  if (chrom < 0 || (u32)chrom >= ctx->nChrom) return refuse(ctx, "gx_push_sequence: a chromosome outside the table");
  if (first % 64) return refuse(ctx, "gx_push_sequence: the first base of a push must be a multiple of 64");
  const u64 len = ctx->len[chrom];
  if (first > len || n > len - first) return refuse(ctx, "gx_push_sequence: bases past the chromosome's length");
  if (n % 64 && first + n != len) return refuse(ctx, "gx_push_sequence: only a chromosome's last push may end inside a word");
  const GcChrom cc = ctx->gcChrom[chrom];
  if (!cc.laid || !n) return GX_OK;   // (skipped, not owned: takes nothing, as tags do)
  hipStream_t s = ctx->stream;
  if (ctx->gcSeq.ensure(GC_PUSH) != hipSuccess) return pool_failed(ctx);
  for (size_t done = 0; done < n;) {
    const size_t take = std::min(n - done, GC_PUSH);
    const int k = ctx->gcStageNext;
    ctx->gcStageNext ^= 1;
    HIPCHECK(ctx->gcStage[k].ensure(GC_PUSH));
    if (!ctx->gcStageFree[k]) HIPCHECK(hipEventCreateWithFlags(&ctx->gcStageFree[k], hipEventDisableTiming));
    else HIPCHECK(hipEventSynchronize(ctx->gcStageFree[k]));   // its previous upload has left the buffer
    memcpy(ctx->gcStage[k].p, bases + done, take);
    HIPCHECK(hipMemcpyAsync(ctx->gcSeq.p, ctx->gcStage[k].p, take, hipMemcpyHostToDevice, s));
    HIPCHECK(hipEventRecord(ctx->gcStageFree[k], s));
    const u64 groups = ((u64)take + 63) / 64 * 4;
    phase_begin(ctx, "gc.pack");
    if (ctx->seqOn)
      hipLaunchKernelGGL(k_seq_pack3, dim3((unsigned)((groups + GC_NT - 1) / GC_NT)), dim3(GC_NT), 0, s, ctx->gcSeq.as<uint4>(), (u64)take,
                         cc.off + (first + done) / 64, ctx->gcVec.as<unsigned long long>(), ctx->gcAcgt.as<unsigned long long>(),
                         ctx->gcAg.as<unsigned long long>());
    else
      hipLaunchKernelGGL(k_gc_pack, dim3((unsigned)((groups + GC_NT - 1) / GC_NT)), dim3(GC_NT), 0, s, ctx->gcSeq.as<uint4>(), (u64)take,
                         cc.off + (first + done) / 64, ctx->gcVec.as<unsigned long long>(), ctx->gcAcgt.as<unsigned long long>());
    if (int rc__ = dbg_sync(ctx, "k_gc_pack")) return rc__;
    HIPCHECK(hipGetLastError());
    phase_end(ctx);
    done += take;
  }
  ctx->gcPushed[chrom] = std::max<uint64_t>(ctx->gcPushed[chrom], first + n);
  ctx->gcDirDirty = true;
  ctx->gcUsed = true;
  return GX_OK;
}

// the rank directory, when bases were pushed since it was built
int gc_dir(gx_ctx* ctx) {
  if (int rc = gc_current(ctx)) return rc;
  if (!ctx->gcDirDirty) return GX_OK;
  const u64 nBlocks = gc_alloc_words(ctx->gcWords) / GC_BLOCK_WORDS;
  phase_begin(ctx, "gc.dir");
  hipLaunchKernelGGL(k_gc_dir_count, dim3((unsigned)((nBlocks + GC_NT - 1) / GC_NT)), dim3(GC_NT), 0, ctx->stream, ctx->gcVec.as<unsigned long long>(),
                     ctx->gcAcgt.as<unsigned long long>(), nBlocks, ctx->gcDir.as<uint2>());
  if (int rc__ = dbg_sync(ctx, "k_gc_dir_count")) return rc__;
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_gc_dir_scan, dim3(std::max(1u, std::min(ctx->nChrom, 1024u))), dim3(GC_DIR_NT), 0, ctx->stream, ctx->gcTab.as<GcChrom>(), ctx->nChrom,
                     ctx->gcDir.as<uint2>());
  if (int rc__ = dbg_sync(ctx, "k_gc_dir_scan")) return rc__;
  HIPCHECK(hipGetLastError());
  phase_end(ctx);
  ctx->gcDirDirty = false;
  ctx->gcUsed = true;
  return GX_OK;
}

// gx_gc_content: n intervals' counts
int gc_content(gx_ctx* ctx, const gx_region* reg, size_t n, uint64_t* outG, uint64_t* outA) {
  static_assert(sizeof(gx_region) == sizeof(GcRegion) && sizeof(gx_region) == 12, "gx_region is the kernel's record");
  if (int rc = gc_dir(ctx)) return rc;
  if (!n) return GX_OK;
  if (n >> 31) return refuse(ctx, "GC content: 2^31 intervals or more");
  hipStream_t s = ctx->stream;
  POOLED(ctx, ctx->gcAux, n * sizeof(GcRegion));
  POOLED(ctx, ctx->gcOut, n * 16);
  HIPCHECK(hipMemcpyAsync(ctx->gcAux.p, reg, n * sizeof(GcRegion), hipMemcpyHostToDevice, s));
  phase_begin(ctx, "gc.content");
  hipLaunchKernelGGL(k_gc_content, dim3((unsigned)((n + GC_NT - 1) / GC_NT)), dim3(GC_NT), 0, s, ctx->gcAux.as<GcRegion>(), (u64)n, ctx->gcTab.as<GcChrom>(),
                     ctx->nChrom, ctx->gcVec.as<unsigned long long>(), ctx->gcAcgt.as<unsigned long long>(), ctx->gcDir.as<uint2>(),
                     ctx->gcOut.as<unsigned long long>(), ctx->gcOut.as<unsigned long long>() + n);
  if (int rc__ = dbg_sync(ctx, "k_gc_content")) return rc__;
  HIPCHECK(hipGetLastError());
  phase_end(ctx);
  HIPCHECK(hipMemcpyAsync(outG, ctx->gcOut.p, n * 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(outA, ctx->gcOut.as<unsigned long long>() + n, n * 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  ctx->gcUsed = true;
  return GX_OK;
}

// the geometry a caller may force (0: the library's choices), each limit with its sentence
int gc_check_geometry(gx_ctx* ctx, unsigned gridE, u32& tile, u64& flush, unsigned gridO) {
  if (tile == 0) tile = GC_TILE;
  if (tile < GC_MIN_TILE || tile > GC_MAX_TILE || tile % 64) return refuse(ctx, "GC bias: a tile must be a multiple of 64 words from 64 to 1024");
  if (flush == 0) flush = GC_FLUSH_WORDS;
  if (flush < tile || flush > GC_FLUSH_WORDS) return refuse(ctx, "GC bias: the flush bound must lie between one tile and 2^25 words");
  if (gridE > GC_MAX_GRID || gridO > GC_MAX_GRID) return refuse(ctx, "GC bias: more than 65535 workgroups");
  return GX_OK;
}

// k_gc_expected over the laid-out chromosomes with in[c]: F[W + 1], and the windows on their bases that are not classed
int gc_expected(gx_ctx* ctx, const std::vector<uint8_t>& in, u32 W, unsigned grid, u32 tile, u64 flush, std::vector<uint64_t>& F, u64* fUn) {
  F.assign((size_t)W + 1, 0);
  *fUn = 0;
  std::vector<GcSpan> spans;
  u64 nTiles = 0, N = 0, walked = 0;
  for (u32 c = 0; c < ctx->nChrom; c++) {
    const GcChrom& cc = ctx->gcChrom[c];
    if (!cc.laid || !in[c]) continue;
    const u32 words = (u32)(((u64)cc.len + 63) / 64);
    spans.push_back(GcSpan{cc.off, words, (u32)nTiles});
    nTiles += (words + tile - 1) / tile;
    N += cc.len;
    walked += words;
  }
  if (spans.empty()) return GX_OK;
  if (nTiles >> 32) return refuse(ctx, "GC bias: 2^32 tiles or more");
  hipStream_t s = ctx->stream;
  const size_t words = GCE_WORDS + (size_t)W + 1;
  POOLED(ctx, ctx->gcAux, spans.size() * sizeof(GcSpan));
  POOLED(ctx, ctx->gcOut, words * 8);
  HIPCHECK(hipMemcpyAsync(ctx->gcAux.p, spans.data(), spans.size() * sizeof(GcSpan), hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemsetAsync(ctx->gcOut.p, 0, words * 8, s));
  GcExpArgs a;
  a.gc = ctx->gcVec.as<unsigned long long>();
  a.acgt = ctx->gcAcgt.as<unsigned long long>();
  a.spans = ctx->gcAux.as<GcSpan>();
  a.nSpan = (u32)spans.size();
  a.nTiles = (u32)nTiles;
  a.T = tile;
  a.W = W;
  a.flushWords = flush;
  a.out = ctx->gcOut.as<unsigned long long>();
  if (grid == 0) grid = (unsigned)std::min<u64>(nTiles, GC_GRID);
  phase_begin(ctx, "gc.expected");
  hipLaunchKernelGGL(k_gc_expected, dim3(std::max(1u, grid)), dim3(GC_NT), gc_exp_lds_bytes(tile, W), s, a);
  if (int rc__ = dbg_sync(ctx, "k_gc_expected")) return rc__;
  HIPCHECK(hipGetLastError());
  phase_end(ctx);
  std::vector<unsigned long long> h(words, 0);
  HIPCHECK(hipMemcpyAsync(h.data(), ctx->gcOut.p, words * 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));   // (the spans' host copy may go)
  ctx->gcUsed = true;
  u64 classed = 0;
  for (u32 g = 0; g <= W; g++) classed += F[g] = h[GCE_WORDS + g];
  if (classed + h[GCE_UNCLASSED] != walked * 64 || classed > N) {
    ctx->err = "GC bias: the classed and the unclassed windows do not add up to the positions walked (a lost or doubled contribution)";
    return GX_ERR_DEVICE;
  }
  *fUn = N - classed;
  return GX_OK;
}

u32 gc_obs_grid(u32 nCk) { return std::max(1u, std::max(std::min(nCk, GC_OBS_GRID), (nCk + CNT_WG_CHUNKS - 1) / CNT_WG_CHUNKS)); }

int gc_obs_refusals(gx_ctx* ctx, u64 n, u64 nCk, u32 grid) {
  if (n >> 31) return refuse(ctx, "GC bias: a sample of 2^31 events or more");
  if ((nCk + CNT_WG_CHUNKS - 1) / CNT_WG_CHUNKS > GC_MAX_GRID) return refuse(ctx, "GC bias: more than 65535 workgroups");
  if (grid && (nCk + grid - 1) / grid > CNT_WG_CHUNKS) return refuse(ctx, "GC bias: a grid that lets a workgroup see more than 272 chunks (its 32-bit counters)");
  return GX_OK;
}

// one sample's observed tables: n events behind the device chunk list dCk[nCk], seen through dCh and its chromosomes by base
int gc_obs_pass(gx_ctx* ctx, const CntChunk* dCk, u32 nCk, const CntChrom* dCh, const IvsBase* dTb, u32 nTb, u64 n, u32 W, u32 grid,
                gx_ctx::GcResult& r) {
  r.Nn.assign((size_t)W + 1, 0);
  r.Nw.assign((size_t)W + 1, 0);
  r.nUn = r.wUn = 0;
  if (!n) return GX_OK;
  hipStream_t s = ctx->stream;
  const size_t words = GCO_WORDS + 2 * ((size_t)W + 1);
  POOLED(ctx, ctx->gcOut, words * 8);
  HIPCHECK(hipMemsetAsync(ctx->gcOut.p, 0, words * 8, s));
  GcObsArgs a;
  a.chunks = dCk;
  a.nChunks = nCk;
  a.chroms = dCh;
  a.nChrom = ctx->nChrom;
  a.bases = dTb;
  a.nBase = nTb;
  a.tab = ctx->gcTab.as<GcChrom>();
  a.gc = ctx->gcVec.as<unsigned long long>();
  a.acgt = ctx->gcAcgt.as<unsigned long long>();
  a.dir = ctx->gcDir.as<uint2>();
  a.W = W;
  a.out = ctx->gcOut.as<unsigned long long>();
  phase_begin(ctx, "gc.observed");
  hipLaunchKernelGGL(k_gc_observed, dim3(grid ? grid : gc_obs_grid(nCk)), dim3(CNT_NT), 2 * ((size_t)W + 1) * 4, s, a);
  if (int rc__ = dbg_sync(ctx, "k_gc_observed")) return rc__;
  HIPCHECK(hipGetLastError());
  phase_end(ctx);
  std::vector<unsigned long long> h(words, 0);
  HIPCHECK(hipMemcpyAsync(h.data(), ctx->gcOut.p, words * 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  ctx->gcUsed = true;
  r.nUn = h[GCO_NUN];
  r.wUn = h[GCO_WUN];
  std::copy(h.begin() + GCO_WORDS, h.begin() + GCO_WORDS + W + 1, r.Nn.begin());
  std::copy(h.begin() + GCO_WORDS + W + 1, h.end(), r.Nw.begin());
  return GX_OK;
}

// every view: the expected table of its set of chromosomes (once per distinct set), then its observed pass
int gc_views(gx_ctx* ctx, const std::vector<KeptView>& views, u32 W, unsigned gridE, u32 tile, u64 flush, u32 gridO, std::vector<gx_ctx::GcResult>& res) {
  const u32 nChrom = ctx->nChrom;
  const std::vector<ViewSize> z = kept_sizes(views);
  // (the refusals come before the staging: nothing is allocated for a call that is refused)
  if (int rc = gc_check_geometry(ctx, gridE, tile, flush, gridO)) return rc;
  for (const ViewSize& v : z)
    if (int rc = gc_obs_refusals(ctx, v.n, v.nCk, gridO)) return rc;
  if (int rc = gc_dir(ctx)) return rc;
  res.assign(views.size(), gx_ctx::GcResult{});
  std::map<std::vector<uint8_t>, size_t> seen;   // a set of chromosomes -> the first view that has it
  for (size_t v = 0; v < views.size(); v++) {
    res[v].W = W;
    std::vector<uint8_t> in(nChrom);
    for (u32 c = 0; c < nChrom; c++) in[c] = ctx->gcChrom[c].laid && (!views[v].save || (*views[v].save)[c]);
    const auto it = seen.find(in);
    if (it != seen.end()) {
      res[v].F = res[it->second].F;
      res[v].fUn = res[it->second].fUn;
      continue;
    }
    if (int rc = gc_expected(ctx, in, W, gridE, tile, flush, res[v].F, &res[v].fUn)) return rc;
    seen.emplace(std::move(in), v);
  }
  std::vector<u32> nTb(views.size());
  const IvsBase* dTb = nullptr;
  return kept_each_view(
      ctx, views, views.size() * std::max(1u, nChrom) * sizeof(IvsBase),
      [&](char* front, const char* dFront) {
        for (size_t v = 0; v < views.size(); v++) nTb[v] = ivs_bases(ctx, views[v], reinterpret_cast<IvsBase*>(front) + v * nChrom);
        dTb = reinterpret_cast<const IvsBase*>(dFront);
      },
      [&](const CntChunk* dCk, u32 nCk, const CntChrom* dCh, size_t v) { return gc_obs_pass(ctx, dCk, nCk, dCh, dTb + v * nChrom, nTb[v], z[v].n, W, gridO, res[v]); });
}

// every kept sample
int gc_bias_kept(gx_ctx* ctx, u32 W) {
  std::vector<gx_ctx::GcResult> res;
  if (int rc = gc_views(ctx, kept_views(ctx), W, 0, 0, 0, 0, res)) return rc;
  kept_stamp(ctx, res);
  ctx->gcRes = std::move(res);
  ctx->gcReady = true;
  return GX_OK;
}

// a caller's host events as one sample whose save mask lists every chromosome
int gc_bias_events(gx_ctx* ctx, const void* ev, size_t n, bool packed, u32 W, unsigned gridE, u32 tile, u64 flush, u32 gridO, gx_ctx::GcResult& r) {
  if (int rc = gc_check_geometry(ctx, gridE, tile, flush, gridO)) return rc;
  if (int rc = gc_obs_refusals(ctx, n, (n + CNT_CHUNK - 1) / CNT_CHUNK, gridO)) return rc;
  std::vector<gx_ctx::Seg> segs;
  if (int rc = kept_upload(ctx, ev, n, packed, segs)) return rc;
  std::vector<gx_ctx::GcResult> res;
  if (int rc = gc_views(ctx, {KeptView{&segs, nullptr}}, W, gridE, tile, flush, gridO, res)) return rc;
  r = std::move(res[0]);
  return GX_OK;
}

// b added to a (a chromosome lives on one context: everything adds)
void gc_add(gx_ctx::GcResult& a, const gx_ctx::GcResult& b) {
  a.fUn += b.fUn;
  a.nUn += b.nUn;
  a.wUn += b.wUn;
  for (size_t g = 0; g < std::min(a.F.size(), b.F.size()); g++) {
    a.F[g] += b.F[g];
    a.Nn[g] += b.Nn[g];
    a.Nw[g] += b.Nw[g];
  }
}

// a result to the caller: min(cap, W + 1) classes of each table
int gc_give(const gx_ctx::GcResult& r, int* rep, int* is_ctrl, int* window, uint64_t* F, uint64_t* f_unclassed, uint64_t* Nn, uint64_t* Nw,
            uint64_t* n_unclassed, uint64_t* w_unclassed, size_t cap) {
  if (cap && (!F || !Nn || !Nw)) return GX_ERR_ORDER;
  if (rep) *rep = r.rep;
  if (is_ctrl) *is_ctrl = r.ctrl ? 1 : 0;
  if (window) *window = (int)r.W;
  if (f_unclassed) *f_unclassed = r.fUn;
  if (n_unclassed) *n_unclassed = r.nUn;
  if (w_unclassed) *w_unclassed = r.wUn;
  if (const size_t k = std::min(cap, r.F.size())) {
    std::copy(r.F.begin(), r.F.begin() + k, F);
    std::copy(r.Nn.begin(), r.Nn.begin() + k, Nn);
    std::copy(r.Nw.begin(), r.Nw.begin() + k, Nw);
  }
  return GX_OK;
}

}  // namespace
