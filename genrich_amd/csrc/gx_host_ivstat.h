// gx_host_ivstat.h -- the host side of gx_interval_stats (gx_ivstat.h): the grid and the list sized for one sample, the one pass
// (and its one rerun with a longer list: gx_host_kept.h counted_list), the read-back, the merged list and the three sums that must agree; the pass over the
// kept samples and the one over a caller's events.  (a part of gx_api.hip's translation unit)
#pragma once
namespace {

// the workgroups of a pass over nCk chunks: at most IVS_GRID, and enough that none sees more than CNT_WG_CHUNKS chunks
u32 ivs_grid(u32 nCk) { return std::max(1u, std::max(std::min(nCk, IVS_GRID), (nCk + CNT_WG_CHUNKS - 1) / CNT_WG_CHUNKS)); }

// what every pass checks before it allocates or launches anything
int ivs_refusals(gx_ctx* ctx, u64 n, u64 nCk, u32 grid, u64 listCap) {
  if (n >> 31) return refuse(ctx, "interval lengths: a sample of 2^31 events or more");
  if (grid > IVS_MAX_GRID || (nCk + CNT_WG_CHUNKS - 1) / CNT_WG_CHUNKS > IVS_MAX_GRID) return refuse(ctx, "interval lengths: more than 65535 workgroups");
  if (grid && (nCk + grid - 1) / grid > CNT_WG_CHUNKS) return refuse(ctx, "interval lengths: a grid that lets a workgroup see more than 272 chunks (its 32-bit counters)");
  if (listCap >> 32) return refuse(ctx, "interval lengths: a list of 2^32 entries or more");
  return GX_OK;
}

// view v's chromosomes by their first position, ascending, into tb[nChrom] (what kept_stage's CntChrom calls active, and not empty)
u32 ivs_bases(const gx_ctx* ctx, const KeptView& view, IvsBase* tb) {
  u32 n = 0;
  for (u32 c = 0; c < ctx->nChrom; c++) {
    const DChrom& d = ctx->hChrom[c];
    tb[c] = IvsBase{0, 0, 0};
    if (!ctx->skip[c] && (!view.save || (*view.save)[c]) && ctx->owned[c] && d.tileBase != NULL_TILE && d.len) tb[n++] = IvsBase{(u64)d.tileBase << TB, c, 0};
  }
  std::sort(tb, tb + n, [](const IvsBase& a, const IvsBase& b) { return a.base < b.base; });
  return n;
}

// one sample: n events behind the device chunk list dCk[nCk], seen through dCh and its chromosomes by base dTb[nTb].
// grid = 0 / listCap = 0: the library's choices.
int ivs_pass(gx_ctx* ctx, const CntChunk* dCk, u32 nCk, const CntChrom* dCh, const IvsBase* dTb, u32 nTb, u64 n, u32 grid, u64 listCap,
             gx_ctx::IvsResult& r) {
  const u32 nChrom = ctx->nChrom;
  r = gx_ctx::IvsResult{};
  r.cn.assign(nChrom, 0);
  r.cw.assign(nChrom, 0);
  r.cb.assign(nChrom, 0);
  if (int rc = ivs_refusals(ctx, n, nCk, grid, listCap)) return rc;
  if (!n) return GX_OK;
  hipStream_t s = ctx->stream;
  const size_t words = IVC_WORDS + 2 * (size_t)IVS_BOUND + 3 * (size_t)nChrom;
  POOLED(ctx, ctx->ivsOut, words * 8);
  std::vector<unsigned long long> h(words, 0);
  IvsArgs a;
  a.chunks = dCk;
  a.nChunks = nCk;
  a.chroms = dCh;
  a.nChrom = nChrom;
  a.bases = dTb;
  a.nBase = nTb;
  a.out = ctx->ivsOut.as<unsigned long long>();
  CountedList list{"interval lengths", "list", &ctx->ivsBig, sizeof(IvsBig), &ctx->ivsOut, words, IVC_STATUS, IVC_NBIG, IVS_ST_LIST_FULL, 0, nullptr,
                   listCap ? listCap : IVS_LIST_CAP};
  phase_begin(ctx, "ivstat");
  if (int rc = counted_list(ctx, list, h, [&](u32 bigCap) -> int {
        a.big = ctx->ivsBig.as<IvsBig>();
        a.bigCap = bigCap;
        hipLaunchKernelGGL(k_ivstat, dim3(grid ? grid : ivs_grid(nCk)), dim3(CNT_NT), 0, s, a);
        if (int rc__ = dbg_sync(ctx, "k_ivstat")) return rc__;
        HIPCHECK(hipGetLastError());
        ctx->ivsUsed = true;
        return GX_OK;
      }))
    return rc;
  phase_end(ctx);
  ctx->ivsLastCap = (size_t)list.cap;
  ctx->ivsLastReruns = list.reruns;
  std::vector<IvsBig> big;
  if (int rc = counted_list_read(ctx, ctx->ivsBig, h[IVC_NBIG], [](const IvsBig& b) { return b.len; }, big)) return rc;
  r.nInv = h[IVC_NINV];
  r.wInv = h[IVC_WINV];
  for (u32 L = 0; L < IVS_BOUND; L++)
    if (h[IVC_WORDS + L]) gx_sparse::append(r.len, {&r.n, &r.w}, L, {h[IVC_WORDS + L], h[IVC_WORDS + IVS_BOUND + L]});
  for (const IvsBig& b : big) gx_sparse::append(r.len, {&r.n, &r.w}, b.len, {b.n, b.w});
  const unsigned long long* gChr = h.data() + IVC_WORDS + 2 * IVS_BOUND;
  u64 sumN = r.nInv, sumW = r.wInv, sumCn = 0, sumCw = 0;
  unsigned __int128 sumB = 0, sumCb = 0;
  for (size_t i = 0; i < r.len.size(); i++) {
    sumN += r.n[i];
    sumW += r.w[i];
    sumB += (unsigned __int128)r.w[i] * r.len[i];
  }
  for (u32 c = 0; c < nChrom; c++) {
    sumCn += r.cn[c] = gChr[c];
    sumCw += r.cw[c] = gChr[nChrom + c];
    sumCb += r.cb[c] = gChr[2 * (size_t)nChrom + c];
  }
  if (sumN != sumCn || sumW != sumCw || sumB != sumCb) {
    ctx->err = "interval lengths: the lengths and the chromosome tallies do not add up to the same intervals";
    return GX_ERR_DEVICE;
  }
  return GX_OK;
}

// the views' chromosomes by base in the staging's front, then every view's pass
int ivs_views(gx_ctx* ctx, const std::vector<KeptView>& views, u32 grid, u64 listCap, std::vector<gx_ctx::IvsResult>& res) {
  const u32 nChrom = ctx->nChrom;
  const std::vector<ViewSize> z = kept_sizes(views);
  // (the refusals come before the staging: nothing is allocated for a call that is refused)
  for (const ViewSize& v : z)
    if (int rc = ivs_refusals(ctx, v.n, v.nCk, grid, listCap)) return rc;
  res.assign(views.size(), gx_ctx::IvsResult{});
  std::vector<u32> nTb(views.size());
  const IvsBase* dTb = nullptr;
  return kept_each_view(
      ctx, views, views.size() * std::max(1u, nChrom) * sizeof(IvsBase),
      [&](char* front, const char* dFront) {
        for (size_t v = 0; v < views.size(); v++) nTb[v] = ivs_bases(ctx, views[v], reinterpret_cast<IvsBase*>(front) + v * nChrom);
        dTb = reinterpret_cast<const IvsBase*>(dFront);
      },
      [&](const CntChunk* dCk, u32 nCk, const CntChrom* dCh, size_t v) { return ivs_pass(ctx, dCk, nCk, dCh, dTb + v * nChrom, nTb[v], z[v].n, grid, listCap, res[v]); });
}

// every kept sample
int ivstat_kept(gx_ctx* ctx) {
  std::vector<gx_ctx::IvsResult> res;
  if (int rc = ivs_views(ctx, kept_views(ctx), 0, 0, res)) return rc;
  kept_stamp(ctx, res);
  ctx->ivs = std::move(res);
  ctx->ivsReady = true;
  return GX_OK;
}

// a caller's host events as one sample whose save mask lists every chromosome
int ivstat_events(gx_ctx* ctx, const gx_event* ev, size_t n, u32 grid, u64 listCap, gx_ctx::IvsResult& r) {
  if (int rc = ivs_refusals(ctx, n, (n + CNT_CHUNK - 1) / CNT_CHUNK, grid, listCap)) return rc;
  std::vector<gx_ctx::Seg> segs;
  if (int rc = kept_upload(ctx, ev, n, false, segs)) return rc;
  std::vector<gx_ctx::IvsResult> res;
  if (int rc = ivs_views(ctx, {KeptView{&segs, nullptr}}, grid, listCap, res)) return rc;
  r = std::move(res[0]);
  return GX_OK;
}

// a result to the caller: min(cap, classes) lengths, min(chrom_cap, chromosomes) tallies
int ivs_give(const gx_ctx::IvsResult& r, int* rep, int* is_ctrl, uint64_t* length, uint64_t* n, uint64_t* w120, size_t cap, size_t* n_classes,
             uint64_t* n_inverted, uint64_t* w120_inverted, uint64_t* cn, uint64_t* cw120, uint64_t* cbases120, size_t chrom_cap) {
  if (rep) *rep = r.rep;
  if (is_ctrl) *is_ctrl = r.ctrl ? 1 : 0;
  if ((cap && (!length || !n || !w120)) || (chrom_cap && (!cn || !cw120 || !cbases120))) return GX_ERR_ORDER;
  if (n_classes) *n_classes = r.len.size();
  if (n_inverted) *n_inverted = r.nInv;
  if (w120_inverted) *w120_inverted = r.wInv;
  if (const size_t k = std::min(cap, r.len.size())) {
    std::copy(r.len.begin(), r.len.begin() + k, length);
    std::copy(r.n.begin(), r.n.begin() + k, n);
    std::copy(r.w.begin(), r.w.begin() + k, w120);
  }
  if (const size_t k = std::min(chrom_cap, r.cn.size())) {
    std::copy(r.cn.begin(), r.cn.begin() + k, cn);
    std::copy(r.cw.begin(), r.cw.begin() + k, cw120);
    std::copy(r.cb.begin(), r.cb.begin() + k, cbases120);
  }
  return GX_OK;
}

// b added to a (the lengths of both ascending; the same chromosome table)
void ivs_add(gx_ctx::IvsResult& a, const gx_ctx::IvsResult& b) {
  a.nInv += b.nInv;
  a.wInv += b.wInv;
  gx_sparse::add(a.len, {&a.n, &a.w}, b.len, {&b.n, &b.w});
  for (size_t c = 0; c < std::min(a.cn.size(), b.cn.size()); c++) {
    a.cn[c] += b.cn[c];
    a.cw[c] += b.cw[c];
    a.cb[c] += b.cb[c];
  }
}

}  // namespace
