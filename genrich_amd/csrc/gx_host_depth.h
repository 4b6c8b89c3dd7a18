// gx_host_depth.h -- the host side of the depth distribution (gx_depth.h): the bases that count, the one pass per closed sample
// (and its one rerun with a longer list: gx_host_kept.h counted_list), the read-back, the sum over contexts.  (a part of gx_api.hip's translation unit)
#pragma once
namespace {

// total = the bases of the chromosomes that count (cov_has_bins), excluded = those of them inside the union of their -E regions,
// clipped to the chromosome: regions may overlap, nest, lie past the end
void depth_domain(const gx_ctx* ctx, u64* total, u64* excluded) {
  u64 T = 0, X = 0;
  std::vector<std::pair<u32, u32>> iv;
  for (u32 c = 0; c < ctx->nChrom; c++) {
    if (!cov_has_bins(ctx, c)) continue;
    const u32 len = ctx->len[c];
    T += len;
    const std::vector<uint32_t>& b = ctx->bed[c];
    iv.clear();
    for (size_t k = 0; k + 1 < b.size(); k += 2) {
      const u32 s = b[k], e = std::min(b[k + 1], len);
      if (s < e) iv.push_back({s, e});
    }
    std::sort(iv.begin(), iv.end());
    u32 upTo = 0;   // (everything below it is accounted for)
    for (const auto& r : iv) {
      const u32 s = std::max(r.first, upTo);
      if (s < r.second) {
        X += r.second - s;
        upTo = r.second;
      }
    }
  }
  *total = T;
  *excluded = X;
}

// the grid of one pass: the knob or the library's choice, and never so few workgroups that a wavefront would walk more than
// DEPTH_WAVE_TILES tiles (the 32-bit LDS counters' bound, gx_depth.h)
u32 depth_grid(const gx_ctx* ctx) {
  const u32 nTiles = ctx->nTiles;
  const u32 all = std::max(1u, (nTiles + DEPTH_NW - 1) / DEPTH_NW);
  const u32 least = (u32)(((u64)nTiles + (u64)DEPTH_NW * DEPTH_WAVE_TILES - 1) / ((u64)DEPTH_NW * DEPTH_WAVE_TILES));
  u32 g = ctx->knob.depthGrid > 0 ? (u32)std::min<long long>(ctx->knob.depthGrid, DEPTH_MAX_GRID) : std::min(all, DEPTH_GRID);
  return std::max(1u, std::max(g, std::min(least, all)));
}

// gx_sample_end, the depth distribution on: one pass over the sample's pileup (pile_input); a second one, with a list of the
// counted size, when the deep list ran full -- the pileup is still where close_sample left it
int depth_sample(gx_ctx* ctx, int isCtrl) {
  hipStream_t s = ctx->stream;
  Pileup& P = isCtrl ? ctx->ctrl : ctx->expt;
  gx_ctx::DepthResult r;
  r.rep = ctx->sample;
  r.ctrl = isCtrl != 0;
  depth_domain(ctx, &r.total, &r.excluded);
  r.bases.assign(DEPTH_BOUND, 0);
  r.rsum.assign(DEPTH_BOUND, 0);
  r.rsq.assign(DEPTH_BOUND, 0);
  const size_t words = DPC_WORDS + 3 * (size_t)DEPTH_BOUND;
  std::vector<unsigned long long> h(words, 0);
  CountedList list{"depth distribution", "deep list", &ctx->depthDeep, sizeof(DepthDeep), &ctx->depthOut, words, DPC_STATUS, DPC_NDEEP, DEPTH_ST_LIST_FULL,
                   DEPTH_ST_NEGATIVE, "depth distribution: a negative pileup", ctx->knob.depthListCap > 0 ? (u64)ctx->knob.depthListCap : DEPTH_LIST_CAP};
  const u32 nTiles = ctx->nTiles;
  if (nTiles && r.total) {
    phase_begin(ctx, isCtrl ? "c.depth" : "t.depth");   // (with -E regions the tight arrays, the zeroing, the pass or the two)
    PileIn in{};
    if (int rc = pile_input(ctx, P, in)) return rc;
    POOLED(ctx, ctx->depthOut, words * 8);
    const u32 grid = depth_grid(ctx);
    if (int rc = counted_list(ctx, list, h, [&](u32 deepCap) -> int {
          if (!ctx->knob.depthPriv)
            hipLaunchKernelGGL(k_depth_hist<false>, dim3(grid), dim3(DEPTH_NW * 64), 0, s, in, nTiles, ctx->depthOut.as<unsigned long long>(),
                               ctx->depthDeep.as<DepthDeep>(), deepCap);
          else
            hipLaunchKernelGGL(k_depth_hist<true>, dim3(grid), dim3(DEPTH_NW * 64), 0, s, in, nTiles, ctx->depthOut.as<unsigned long long>(),
                               ctx->depthDeep.as<DepthDeep>(), deepCap);
          if (int rc__ = dbg_sync(ctx, "k_depth_hist")) return rc__;
          HIPCHECK(hipGetLastError());
          return GX_OK;
        }))
      return rc;
    phase_end(ctx);
    ctx->depthUsed = true;
  }
  ctx->depthLastCap = (size_t)list.cap;
  ctx->depthLastReruns = list.reruns;
  std::vector<DepthDeep> deep;
  if (int rc = counted_list_read(ctx, ctx->depthDeep, h[DPC_NDEEP], [](const DepthDeep& d) { return d.v; }, deep)) return rc;
  u64 covered = 0;
  for (u32 d = 0; d < DEPTH_BOUND; d++) {
    r.bases[d] = h[DPC_WORDS + d];
    r.rsum[d] = h[DPC_WORDS + DEPTH_BOUND + d];
    r.rsq[d] = h[DPC_WORDS + 2 * (size_t)DEPTH_BOUND + d];
    covered += r.bases[d];
  }
  for (const DepthDeep& d : deep) {
    covered += d.bases;
    gx_sparse::append(r.deepV, {&r.deepBases}, d.v, {d.bases});
  }
  r.maxV = h[DPC_VMAX];
  r.minV = covered ? (u64)(u32)~(u32)h[DPC_VMININV] : 0;
  const u64 B = r.total - r.excluded;
  if (covered > B) {
    ctx->err = "depth distribution: more covered bases than bases (a lost or doubled contribution)";
    return GX_ERR_ARR;
  }
  r.zero = B - covered;
  ctx->depth.push_back(std::move(r));
  return GX_OK;
}

// gx_reset: the results go, the buffers stay with the context
void drop_depth(gx_ctx* ctx) {
  ctx->depth.clear();
  ctx->depthUsed = false;
}

// b added to a: the classes add, the deep lists merge (both ascending in v)
void depth_add(gx_ctx::DepthResult& a, const gx_ctx::DepthResult& b) {
  a.total += b.total;
  a.excluded += b.excluded;
  a.zero += b.zero;
  a.maxV = std::max(a.maxV, b.maxV);
  a.minV = !a.minV ? b.minV : !b.minV ? a.minV : std::min(a.minV, b.minV);
  for (u32 d = 0; d < DEPTH_BOUND; d++) {
    a.bases[d] += b.bases[d];
    a.rsum[d] += b.rsum[d];
    a.rsq[d] += b.rsq[d];
  }
  gx_sparse::add(a.deepV, {&a.deepBases}, b.deepV, {&b.deepBases});
}

// a result to the caller: the three arrays whole (DEPTH_BOUND entries each, where asked for), min(cap, entries) deep pairs
int depth_give(const gx_ctx::DepthResult& r, gx_depth_hist* out, uint64_t* bases, uint64_t* rsum, uint64_t* rsq, uint64_t* deep_v,
               uint64_t* deep_bases, size_t cap, size_t* n_deep) {
  if (cap && (!deep_v || !deep_bases)) return GX_ERR_ORDER;
  if (out) {
    *out = gx_depth_hist{};
    out->rep = r.rep;
    out->is_ctrl = r.ctrl ? 1 : 0;
    out->total = r.total;
    out->excluded = r.excluded;
    out->zero = r.zero;
    out->min_v = r.minV;
    out->max_v = r.maxV;
    out->bases = bases;
    out->rsum = rsum;
    out->rsq = rsq;
    out->deep_v = deep_v;
    out->deep_bases = deep_bases;
    out->n_deep = std::min(cap, r.deepV.size());
  }
  if (bases) std::copy(r.bases.begin(), r.bases.end(), bases);
  if (rsum) std::copy(r.rsum.begin(), r.rsum.end(), rsum);
  if (rsq) std::copy(r.rsq.begin(), r.rsq.end(), rsq);
  if (n_deep) *n_deep = r.deepV.size();
  const size_t n = std::min(cap, r.deepV.size());
  if (n) {
    std::copy(r.deepV.begin(), r.deepV.begin() + n, deep_v);
    std::copy(r.deepBases.begin(), r.deepBases.begin() + n, deep_bases);
  }
  return GX_OK;
}

}  // namespace
