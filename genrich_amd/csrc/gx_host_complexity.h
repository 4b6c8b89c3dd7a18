// gx_host_complexity.h -- the host side of gx_complexity (gx_complexity.h): the table sized for one sample, the two kernels,
// the read-back and the sparse histogram; the pass over the kept samples and the one over a caller's events.
// (a part of gx_api.hip's translation unit)
#pragma once
namespace {

// the smallest table a sample of n events takes: a power of two of at least 2 n slots (and 2)
int cpx_least_cap_log(u64 n) {
  int lg = 1;
  while (((u64)1 << lg) < 2 * n) lg++;
  return lg;
}

// what every pass checks before it allocates or launches anything: the key's 32 bits hold every start in tile space
int cpx_domain(gx_ctx* ctx) {
  if (((u64)ctx->nTiles << TB) > CPX_MAX_SPACE)
    return refuse(ctx, "library complexity: a genome of more than 2^32 - 1 bases in tile space does not fit the 64-bit key");
  return GX_OK;
}

// one sample: n events behind the device chunk list dCk[nCk], seen through the device chromosome view dCh -> N, D and the
// (multiplicity, keys) pairs, ascending.  grid = 0 / capLog = 0: the library's choices.
int cpx_pass(gx_ctx* ctx, const CntChunk* dCk, u32 nCk, const CntChrom* dCh, u64 n, u32 grid, int capLog, gx_ctx::CpxResult& r) {
  r = gx_ctx::CpxResult{};
  if (n >> 31) return refuse(ctx, "library complexity: a sample of 2^31 events or more");
  const int least = cpx_least_cap_log(n);
  if (!capLog) capLog = least;
  if (capLog < least || capLog > 32) return refuse(ctx, "library complexity: a table of fewer than 2 n slots (or more than 2^32)");
  if (grid > CPX_MAX_GRID) return refuse(ctx, "library complexity: more than 65535 workgroups");
  if (!n) return GX_OK;
  hipStream_t s = ctx->stream;
  const u64 cap = (u64)1 << capLog;
  const u32 bigCap = (u32)(n / CPX_BOUND);
  const size_t ctlWords = CPXC_WORDS + CPX_BOUND;
  POOLED(ctx, ctx->cpxTab, cap * sizeof(CpxSlot));
  POOLED(ctx, ctx->cpxCtl, ctlWords * 8);
  POOLED(ctx, ctx->cpxBig, (size_t)std::max(1u, bigCap) * 4);
  CpxArgs a;
  a.chunks = dCk;
  a.nChunks = nCk;
  a.chroms = dCh;
  a.nChrom = ctx->nChrom;
  a.T.slot = ctx->cpxTab.as<CpxSlot>();
  a.T.mask = (u32)(cap - 1);
  a.T.ctl = ctx->cpxCtl.as<unsigned long long>();
  unsigned long long* dHist = a.T.ctl + CPXC_WORDS;
  phase_begin(ctx, "cpx_insert");
  HIPCHECK(hipMemsetAsync(a.T.slot, 0, cap * sizeof(CpxSlot), s));
  HIPCHECK(hipMemsetAsync(a.T.ctl, 0, ctlWords * 8, s));
  hipLaunchKernelGGL(k_cpx_insert, dim3(grid ? grid : std::max(1u, std::min(nCk, CPX_GRID))), dim3(CPX_NT), 0, s, a);
  if (int rc__ = dbg_sync(ctx, "k_cpx_insert")) return rc__;
  phase_end(ctx);
  HIPCHECK(hipGetLastError());
  ctx->cpxUsed = true;
  ctx->cpxLastCapLog = (u32)capLog;
  phase_begin(ctx, "cpx_hist");
  const u32 hGrid = grid ? grid : (u32)std::max<u64>(1, std::min<u64>((cap + CPX_HIST_NT - 1) / CPX_HIST_NT, CPX_HIST_GRID));
  hipLaunchKernelGGL(k_cpx_hist, dim3(hGrid), dim3(CPX_HIST_NT), 0, s, a.T, dHist, ctx->cpxBig.as<u32>(), bigCap);
  if (int rc__ = dbg_sync(ctx, "k_cpx_hist")) return rc__;
  phase_end(ctx);
  HIPCHECK(hipGetLastError());
  std::vector<unsigned long long> h(ctlWords);
  HIPCHECK(hipMemcpyAsync(h.data(), a.T.ctl, ctlWords * 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (h[CPXC_STATUS]) {   // (a bounded loop ran out: it cannot with at least 2 n slots and n / CPX_BOUND list entries)
    ctx->err = (h[CPXC_STATUS] & CPX_ST_TABLE_FULL) ? "library complexity: the table ran full" : "library complexity: the list of frequent keys ran full";
    return GX_ERR_DEVICE;
  }
  std::vector<u32> big;
  if (int rc = counted_list_read(ctx, ctx->cpxBig, h[CPXC_NBIG], [](u32 m) { return m; }, big)) return rc;
  r.N = h[CPXC_N];
  r.D = h[CPXC_D];
  u64 sumH = 0, sumMH = 0;
  for (u32 m = 1; m < CPX_BOUND; m++)
    if (h[CPXC_WORDS + m]) gx_sparse::append(r.mult, {&r.keys}, m, {h[CPXC_WORDS + m]});
  for (u32 m : big) gx_sparse::append(r.mult, {&r.keys}, m, {1});
  for (size_t i = 0; i < r.mult.size(); i++) {
    sumH += r.keys[i];
    sumMH += r.mult[i] * r.keys[i];
  }
  if (sumH != r.D || sumMH != r.N) {
    ctx->err = "library complexity: the histogram does not add up to the keys and the observations";
    return GX_ERR_DEVICE;
  }
  return GX_OK;
}

// every kept sample
int complexity_kept(gx_ctx* ctx) {
  if (int rc = cpx_domain(ctx)) return rc;
  const std::vector<KeptView> views = kept_views(ctx);
  const std::vector<ViewSize> z = kept_sizes(views);
  for (const ViewSize& v : z)
    if (v.n >> 31) return refuse(ctx, "library complexity: a sample of 2^31 events or more");
  std::vector<gx_ctx::CpxResult> res(views.size());
  if (int rc = kept_each_view(ctx, views, [&](const CntChunk* dCk, u32 nCk, const CntChrom* dCh, size_t v) { return cpx_pass(ctx, dCk, nCk, dCh, z[v].n, 0, 0, res[v]); }))
    return rc;
  kept_stamp(ctx, res);
  ctx->cpx = std::move(res);
  ctx->cpxReady = true;
  return GX_OK;
}

// a caller's host events as one sample whose save mask lists every chromosome
int complexity_events(gx_ctx* ctx, const gx_event* ev, size_t n, u32 grid, int capLog, gx_ctx::CpxResult& r) {
  if (int rc = cpx_domain(ctx)) return rc;
  // (the refusals that depend on n alone come before the upload: nothing is allocated for a call that is refused)
  if ((u64)n >> 31) return refuse(ctx, "library complexity: a sample of 2^31 events or more");
  if (capLog && (capLog < cpx_least_cap_log(n) || capLog > 32)) return refuse(ctx, "library complexity: a table of fewer than 2 n slots (or more than 2^32)");
  if (grid > CPX_MAX_GRID) return refuse(ctx, "library complexity: more than 65535 workgroups");
  std::vector<gx_ctx::Seg> segs;
  if (int rc = kept_upload(ctx, ev, n, false, segs)) return rc;
  return kept_each_view(ctx, {KeptView{&segs, nullptr}}, [&](const CntChunk* dCk, u32 nCk, const CntChrom* dCh, size_t) { return cpx_pass(ctx, dCk, nCk, dCh, n, grid, capLog, r); });
}

// a result to the caller: min(cap, classes) pairs
int cpx_give(const gx_ctx::CpxResult& r, int* rep, int* is_ctrl, uint64_t* n_obs, uint64_t* n_distinct, uint64_t* mult, uint64_t* keys, size_t cap,
             size_t* n_classes) {
  if (rep) *rep = r.rep;
  if (is_ctrl) *is_ctrl = r.ctrl ? 1 : 0;
  if (cap && (!mult || !keys)) return GX_ERR_ORDER;
  if (n_obs) *n_obs = r.N;
  if (n_distinct) *n_distinct = r.D;
  if (n_classes) *n_classes = r.mult.size();
  const size_t n = std::min(cap, r.mult.size());
  if (n) {
    std::copy(r.mult.begin(), r.mult.begin() + n, mult);
    std::copy(r.keys.begin(), r.keys.begin() + n, keys);
  }
  return GX_OK;
}

// b's pairs added to a's (both ascending in the multiplicity)
void cpx_add(gx_ctx::CpxResult& a, const gx_ctx::CpxResult& b) {
  a.N += b.N;
  a.D += b.D;
  gx_sparse::add(a.mult, {&a.keys}, b.mult, {&b.keys});
}

}  // namespace
