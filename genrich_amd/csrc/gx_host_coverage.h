// gx_host_coverage.h -- the host side of the binned coverage (gx_coverage.h): the bins' layout, the one pass per closed sample,
// the read-back.  (a part of gx_api.hip's translation unit)
#pragma once
namespace {

// a chromosome has bins on this context iff the context computes it: not skipped (-e), not empty, owned (layout_tiles' rule)
bool cov_has_bins(const gx_ctx* ctx, u32 c) { return !ctx->skip[c] && ctx->owned[c] && ctx->len[c] != 0; }

// first bin of every chromosome in a sample's array, and the device's copy of it; after gx_set_coverage_bins, and again when
// gx_set_chroms / gx_set_owned has changed the table since
int cov_layout(gx_ctx* ctx) {
  const u32 W = ctx->covW, n = ctx->nChrom;
  ctx->covOff.assign((size_t)n + 1, 0);
  std::vector<u32> first((size_t)n + 1, 0);
  u64 at = 0;
  for (u32 c = 0; c < n; c++) {
    ctx->covOff[c] = (size_t)at;
    first[c] = (u32)std::min<u64>(at, COV_MAX_BINS);
    if (cov_has_bins(ctx, c)) at += ((u64)ctx->len[c] + W - 1) / W;
  }
  ctx->covOff[n] = (size_t)at;
  first[n] = (u32)std::min<u64>(at, COV_MAX_BINS);
  if (at > COV_MAX_BINS) {
    ctx->err = "more than 2^30 coverage bins";
    return GX_ERR_ORDER;
  }
  HIPCHECK(ctx->covChromBin.ensure(((size_t)n + 1) * 4));
  HIPCHECK(hipMemcpy(ctx->covChromBin.p, first.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice));
  ctx->covDirty = false;
  return GX_OK;
}

// The closed sample's pileup as all three passes over it read it (gx_pileup.h: k_cov_bins, k_depth_hist, k_profile), where
// close_sample left it.  Nothing has stashed, merged or reused the loose slots yet; with -E regions the tight arrays are read
// (pack_pileup, which runs once per pileup however many passes ask: what the control merge needs there anyway -- no carry says
// V_MARK).  chromBin stays the coverage's.
int pile_input(gx_ctx* ctx, Pileup& P, PileIn& in) {
  in.tileIvOff = P.tileIvOff.as<u32>();
  in.tileChrom = ctx->dTileChrom.as<u32>();
  in.nChrom = ctx->nChrom;
  if (ctx->hasBed) {
    if (int rc = pack_pileup(ctx, P)) return rc;
    in.end = P.ivEnd.as<u32>(); in.v = P.ivV.as<int>(); in.meta = ctx->tileMeta.as<TileMeta>(); in.loose = 0u;
  } else if (P.inLoose) {   // (a control: scan_and_close has stashed it for its merge)
    in.end = P.looseEnd.as<u32>(); in.v = P.looseV.as<int>(); in.meta = P.meta.as<TileMeta>(); in.loose = 1u;
  } else {
    in.end = ctx->looseEnd.as<u32>(); in.v = ctx->looseV.as<int>(); in.meta = ctx->tileMeta.as<TileMeta>(); in.loose = 1u;
  }
  return GX_OK;
}

// gx_sample_end, coverage on: the sample's pileup (pile_input) summed into a bin array of its own
int cov_sample(gx_ctx* ctx, int isCtrl) {
  if (ctx->covDirty)
    if (int rc = cov_layout(ctx)) return rc;
  hipStream_t s = ctx->stream;
  Pileup& P = isCtrl ? ctx->ctrl : ctx->expt;
  gx_ctx::CovSample cs;
  cs.rep = ctx->sample;
  cs.ctrl = isCtrl != 0;
  const size_t nBins = ctx->covOff[ctx->nChrom];
  POOLED(ctx, cs.bins, std::max<size_t>(nBins, 1) * 8);
  if (nBins) {
    phase_begin(ctx, isCtrl ? "c.cover" : "t.cover");   // (the zeroing, with -E regions the tight arrays, the pass)
    HIPCHECK(hipMemsetAsync(cs.bins.p, 0, nBins * 8, s));
    PileIn in{};
    if (int rc = pile_input(ctx, P, in)) return rc;
    in.chromBin = ctx->covChromBin.as<u32>();
    const u32 nTiles = ctx->nTiles;
    hipLaunchKernelGGL(k_cov_bins, dim3(std::max(1u, std::min((nTiles + COV_NW - 1) / COV_NW, (u32)(8 * ctx->numCU)))), dim3(COV_NW * 64), 0, s,
                       in, nTiles, ctx->covW, cs.bins.as<unsigned long long>());
    if (int rc__ = dbg_sync(ctx, "k_cov_bins")) return rc__;
    phase_end(ctx);
    HIPCHECK(hipGetLastError());
  }
  ctx->cov.push_back(std::move(cs));
  return GX_OK;
}

// gx_reset: the results go, their buffers stay with the context
void drop_coverage(gx_ctx* ctx) {
  for (gx_ctx::CovSample& c : ctx->cov) recycle(ctx, c.bins);
  ctx->cov.clear();
}

}  // namespace
