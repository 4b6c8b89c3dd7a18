// gx_host_ivstat.h -- the host side of gx_interval_stats (gx_ivstat.h): the grid and the list sized for one sample, the one pass
// (and its one rerun with a longer list), the read-back, the merged list and the three sums that must agree; the pass over the
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
  u64 cap = listCap ? listCap : IVS_LIST_CAP;
  u32 reruns = 0;
  IvsArgs a;
  a.chunks = dCk;
  a.nChunks = nCk;
  a.chroms = dCh;
  a.nChrom = nChrom;
  a.bases = dTb;
  a.nBase = nTb;
  a.out = ctx->ivsOut.as<unsigned long long>();
  phase_begin(ctx, "ivstat");
  for (;;) {
    if (cap >> 32) return refuse(ctx, "interval lengths: a list of 2^32 entries or more");
    POOLED(ctx, ctx->ivsBig, (size_t)cap * sizeof(IvsBig));
    a.big = ctx->ivsBig.as<IvsBig>();
    a.bigCap = (u32)cap;
    HIPCHECK(hipMemsetAsync(a.out, 0, words * 8, s));
    hipLaunchKernelGGL(k_ivstat, dim3(grid ? grid : ivs_grid(nCk)), dim3(CNT_NT), 0, s, a);
    if (int rc__ = dbg_sync(ctx, "k_ivstat")) return rc__;
    HIPCHECK(hipGetLastError());
    ctx->ivsUsed = true;
    HIPCHECK(hipMemcpyAsync(h.data(), a.out, words * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (!(h[IVC_STATUS] & IVS_ST_LIST_FULL)) break;
    if (reruns || h[IVC_NBIG] <= cap) {   // (the counted size holds every entry: one rerun always suffices)
      ctx->err = "interval lengths: the list ran full twice";
      return GX_ERR_DEVICE;
    }
    cap = h[IVC_NBIG];
    reruns++;
  }
  phase_end(ctx);
  ctx->ivsLastCap = (size_t)cap;
  ctx->ivsLastReruns = reruns;
  const u64 nBig = h[IVC_NBIG];
  std::vector<IvsBig> big((size_t)nBig);
  if (nBig) {
    HIPCHECK(hipMemcpyAsync(big.data(), ctx->ivsBig.p, (size_t)nBig * sizeof(IvsBig), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    std::sort(big.begin(), big.end(), [](const IvsBig& x, const IvsBig& y) { return x.len < y.len; });   // (the list comes in the order of the races)
  }
  r.nInv = h[IVC_NINV];
  r.wInv = h[IVC_WINV];
  for (u32 L = 0; L < IVS_BOUND; L++)
    if (h[IVC_WORDS + L]) {
      r.len.push_back(L);
      r.n.push_back(h[IVC_WORDS + L]);
      r.w.push_back(h[IVC_WORDS + IVS_BOUND + L]);
    }
  for (const IvsBig& b : big) {
    if (!r.len.empty() && r.len.back() == b.len) {
      r.n.back() += b.n;
      r.w.back() += b.w;
    } else {
      r.len.push_back(b.len);
      r.n.push_back(b.n);
      r.w.push_back(b.w);
    }
  }
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

// the views' chromosome tables behind kept_stage's front, then every view's pass
int ivs_views(gx_ctx* ctx, const std::vector<KeptView>& views, const std::vector<u64>& nEv, u32 grid, u64 listCap, std::vector<gx_ctx::IvsResult>& res) {
  const u32 nChrom = ctx->nChrom;
  // (the refusals come before the staging: nothing is allocated for a call that is refused)
  for (size_t v = 0; v < views.size(); v++) {
    u64 nCk = 0;
    for (const gx_ctx::Seg& sg : *views[v].segs) nCk += (sg.n + CNT_CHUNK - 1) / CNT_CHUNK;
    if (int rc = ivs_refusals(ctx, nEv[v], nCk, grid, listCap)) return rc;
  }
  KeptIn in;
  if (int rc = kept_stage(ctx, views, views.size() * std::max(1u, nChrom) * sizeof(IvsBase), true, false, in)) return rc;
  IvsBase* tb = reinterpret_cast<IvsBase*>(in.front);
  std::vector<u32> nTb(views.size());
  for (size_t v = 0; v < views.size(); v++) nTb[v] = ivs_bases(ctx, views[v], tb + v * nChrom);
  if (int rc = kept_send(ctx, in)) return rc;
  HIPCHECK(hipStreamSynchronize(ctx->stream));   // (a sample without events launches nothing: the staging area is free again)
  res.assign(views.size(), gx_ctx::IvsResult{});
  const IvsBase* dTb = reinterpret_cast<const IvsBase*>(in.dFront);
  for (size_t v = 0; v < views.size(); v++)
    if (int rc = ivs_pass(ctx, in.dCk + in.chunk0[v], (u32)(in.chunk0[v + 1] - in.chunk0[v]), in.dCh + v * nChrom, dTb + v * nChrom, nTb[v], nEv[v],
                          grid, listCap, res[v]))
      return rc;
  return GX_OK;
}

// every kept sample, through the staging the passes share (gx_host_count.h kept_stage)
int ivstat_kept(gx_ctx* ctx) {
  const size_t nS = ctx->kept.size();
  std::vector<u64> nEv(nS, 0);
  for (size_t k = 0; k < nS; k++)
    for (const gx_ctx::Seg& sg : ctx->kept[k].segs) nEv[k] += sg.n;
  std::vector<gx_ctx::IvsResult> res;
  if (int rc = ivs_views(ctx, kept_views(ctx), nEv, 0, 0, res)) return rc;
  for (size_t k = 0; k < nS; k++) {
    res[k].rep = ctx->kept[k].rep;
    res[k].ctrl = ctx->kept[k].ctrl;
  }
  ctx->ivs = std::move(res);
  ctx->ivsReady = true;
  return GX_OK;
}

// a caller's host events as one sample whose save mask lists every chromosome
int ivstat_events(gx_ctx* ctx, const gx_event* ev, size_t n, u32 grid, u64 listCap, gx_ctx::IvsResult& r) {
  if (int rc = ivs_refusals(ctx, n, (n + CNT_CHUNK - 1) / CNT_CHUNK, grid, listCap)) return rc;
  std::vector<gx_ctx::Seg> segs;
  if (n) {
    POOLED(ctx, ctx->ivsEv, n * sizeof(gx_event));
    HIPCHECK(hipMemcpyAsync(ctx->ivsEv.p, ev, n * sizeof(gx_event), hipMemcpyHostToDevice, ctx->stream));
    segs.push_back({ctx->ivsEv.as<gx_event>(), n, nullptr, false});
  }
  std::vector<gx_ctx::IvsResult> res;
  if (int rc = ivs_views(ctx, {KeptView{&segs, nullptr}}, {(u64)n}, grid, listCap, res)) return rc;
  r = std::move(res[0]);
  return GX_OK;
}

// a result to the caller: min(cap, classes) lengths, min(chrom_cap, chromosomes) tallies
int ivs_give(const gx_ctx::IvsResult& r, uint64_t* length, uint64_t* n, uint64_t* w120, size_t cap, size_t* n_classes, uint64_t* n_inverted,
             uint64_t* w120_inverted, uint64_t* cn, uint64_t* cw120, uint64_t* cbases120, size_t chrom_cap) {
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
  gx_ctx::IvsResult o;
  o.rep = a.rep;
  o.ctrl = a.ctrl;
  o.nInv = a.nInv + b.nInv;
  o.wInv = a.wInv + b.wInv;
  size_t i = 0, j = 0;
  while (i < a.len.size() || j < b.len.size()) {
    const bool ta = j == b.len.size() || (i < a.len.size() && a.len[i] <= b.len[j]);
    const bool tb = i == a.len.size() || (j < b.len.size() && b.len[j] <= a.len[i]);
    o.len.push_back(ta ? a.len[i] : b.len[j]);
    o.n.push_back((ta ? a.n[i] : 0) + (tb ? b.n[j] : 0));
    o.w.push_back((ta ? a.w[i] : 0) + (tb ? b.w[j] : 0));
    i += ta;
    j += tb;
  }
  o.cn = b.cn;
  o.cw = b.cw;
  o.cb = b.cb;
  for (size_t c = 0; c < std::min(a.cn.size(), b.cn.size()); c++) {
    o.cn[c] += a.cn[c];
    o.cw[c] += a.cw[c];
    o.cb[c] += a.cb[c];
  }
  a = std::move(o);
}

}  // namespace
