// gx_host_profile.h -- the host side of the profiles around anchors (gx_profile.h): the anchor table's device copy, the one
// pass per closed sample, the read-back.  (a part of gx_api.hip's translation unit)
#pragma once
namespace {

// the anchors as the kernel wants them: the first tile of each one's chromosome, or NULL_TILE where this context computes
// nothing (cov_has_bins' rule; an index behind the table); after gx_set_profile, and again when gx_set_chroms / gx_set_owned
// has changed the layout since
int prof_layout(gx_ctx* ctx) {
  const size_t n = ctx->profAnchors.size();
  std::vector<ProfAnchor> tab(n);
  for (size_t i = 0; i < n; i++) {
    const gx_anchor& a = ctx->profAnchors[i];
    const bool live = a.chrom < ctx->nChrom && cov_has_bins(ctx, a.chrom) && ctx->hChrom[a.chrom].tileBase != NULL_TILE;
    tab[i] = ProfAnchor{live ? ctx->hChrom[a.chrom].tileBase : NULL_TILE, a.pos, a.strand, live ? ctx->len[a.chrom] : 0u};
  }
  HIPCHECK(ctx->profDev.ensure(std::max<size_t>(n, 1) * sizeof(ProfAnchor)));
  if (n) HIPCHECK(hipMemcpy(ctx->profDev.p, tab.data(), n * sizeof(ProfAnchor), hipMemcpyHostToDevice));
  ctx->profDirty = false;
  return GX_OK;
}

// gx_sample_end, profile on: the sample's pileup, where close_sample left it (pile_input's three forms), summed around every
// anchor -- the aggregate always, the matrix when one is kept
int prof_sample(gx_ctx* ctx, int isCtrl) {
  if (ctx->profDirty)
    if (int rc = prof_layout(ctx)) return rc;
  hipStream_t s = ctx->stream;
  Pileup& P = isCtrl ? ctx->ctrl : ctx->expt;
  const u32 nA = (u32)ctx->profAnchors.size(), nb = ctx->profNb;
  const u32 grid = std::max(1u, std::min((nA + PROF_NW - 1) / PROF_NW, (u32)(4 * ctx->numCU)));
  gx_ctx::ProfSample ps;
  ps.rep = ctx->sample;
  ps.ctrl = isCtrl != 0;
  if (pooled(ctx, ps.agg, (size_t)nb * 8) != hipSuccess || (ctx->profKeep && pooled(ctx, ps.cells, (size_t)nA * nb * 8) != hipSuccess) ||
      pooled(ctx, ctx->profPartial, (size_t)grid * nb * 8) != hipSuccess) {
    recycle(ctx, ps.agg);
    recycle(ctx, ps.cells);
    return pool_failed(ctx);
  }
  phase_begin(ctx, isCtrl ? "c.profile" : "t.profile");   // (with -E regions the tight arrays, the pass, the column sums)
  PileIn in{};
  if (int rc = pile_input(ctx, P, in)) return rc;
  hipLaunchKernelGGL(k_profile, dim3(grid), dim3(PROF_NW * 64), 0, s, in, ctx->nTiles, ctx->profDev.as<ProfAnchor>(), nA, ctx->profF,
                     ctx->profB, nb, ctx->profKeep ? ps.cells.as<unsigned long long>() : nullptr,
                     ctx->profPartial.as<unsigned long long>());
  if (int rc__ = dbg_sync(ctx, "k_profile")) return rc__;
  hipLaunchKernelGGL(k_profile_sum, dim3((nb + 63) / 64), dim3(256), 0, s, ctx->profPartial.as<unsigned long long>(), grid, nb,
                     ps.agg.as<unsigned long long>());
  if (int rc__ = dbg_sync(ctx, "k_profile_sum")) return rc__;
  phase_end(ctx);
  HIPCHECK(hipGetLastError());
  ctx->prof.push_back(std::move(ps));
  return GX_OK;
}

// gx_reset: the results go, their buffers stay with the context
void drop_profile(gx_ctx* ctx) {
  for (gx_ctx::ProfSample& p : ctx->prof) {
    recycle(ctx, p.agg);
    recycle(ctx, p.cells);
  }
  ctx->prof.clear();
}

}  // namespace
