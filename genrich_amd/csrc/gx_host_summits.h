// gx_host_summits.h -- the host side of gx_peak_summits (gx_summits.h): the pooled peak space from the treatments' scatters
// (gx_host_peaksig.h's staging), k_summits and its second launch for the peaks whose runs do not fit a wavefront's LDS, the
// list that is counted and read once more when it ran full; the pass over the kept treatments and the one over a caller's
// events and peaks.
// (a part of gx_api.hip's translation unit)
#pragma once
namespace {

static_assert(sizeof(SumRec) == sizeof(gx_summit) && offsetof(SumRec, height) == offsetof(gx_summit, height120) &&
              offsetof(SumRec, prom) == offsetof(gx_summit, prominence120), "SumRec is gx_summit");

u64 sum_list_cap(size_t nPk) { return std::max<u64>(SUM_LIST_MIN, 2 * (u64)nPk); }

// the summits of the views' pooled depth in the peaks pkv[nPk] -> res, ascending in (peak, pos).
// grid = 0: the library's geometry, else that many workgroups for every kernel; runCap / listCap = 0: the library's.
int sum_pass(gx_ctx* ctx, const std::vector<KeptView>& views, const PsigPeak* pkv, size_t nPk, u32 pPct, u32 rPct, u32 grid, u32 runCap, u64 listCap,
             std::vector<gx_summit>& res) {
  hipStream_t s = ctx->stream;
  const u32 nS = (u32)views.size();
  res.clear();
  ctx->sumLastReruns = ctx->sumLastBig = 0;
  if (nPk >= 0xFFFFFFF0ull) {
    ctx->err = "too many peaks to take the summits in";
    return GX_ERR_MEM;
  }
  if (!nS || !nPk) return GX_OK;
  PsigStaged st;
  if (int rc = psig_stage(ctx, views, pkv, nPk, "summits", st)) return rc;
  // the pooled space: cleared once, every view's difference array added
  HIPCHECK(hipMemsetAsync(ctx->psigSpace.p, 0, (size_t)st.slots * 4, s));
  for (u32 k = 0; k < nS; k++)
    if (int rc = psig_scatter(ctx, st, k, grid)) return rc;
  POOLED(ctx, ctx->sumOut, SMC_WORDS * 8);
  POOLED(ctx, ctx->sumFlag, nPk * 4);
  SumArgs a{};
  a.space = ctx->psigSpace.as<int>();
  a.off = st.dOff;
  a.pk = st.dPk;
  a.nPk = (u32)nPk;
  a.P = pPct;
  a.R = rPct;
  a.runCap = runCap ? std::min(runCap, SUM_RUN_CAP) : SUM_RUN_CAP;
  a.out = ctx->sumOut.as<unsigned long long>();
  const u32 wpb = SUM_NT / 64;
  const u32 grid1 = grid ? grid : std::max(1u, std::min((u32)((nPk + wpb - 1) / wpb), SUM_GRID));
  std::vector<unsigned long long> h(SMC_WORDS, 0);
  std::vector<u32> flags;
  std::vector<SumBig> big;
  CountedList list{"peak summits", "summit list", &ctx->sumList, sizeof(SumRec), &ctx->sumOut, SMC_WORDS, SMC_STATUS, SMC_COUNT, SUM_ST_LIST_FULL,
                   SUM_ST_RUNS, "peak summits: a peak with more runs than were counted", listCap ? listCap : sum_list_cap(nPk)};
  if (int rc = counted_list(ctx, list, h, [&](u32 cap) -> int {
        a.list = ctx->sumList.as<SumRec>();
        a.listCap = cap;
        a.flag = ctx->sumFlag.as<u32>();
        a.big = nullptr;
        a.nBig = 0;
        HIPCHECK(hipMemsetAsync(a.flag, 0, nPk * 4, s));
        hipLaunchKernelGGL(k_summits<false>, dim3(grid1), dim3(SUM_NT), 0, s, a);
        if (int rc__ = dbg_sync(ctx, "k_summits")) return rc__;
        // the peaks with more runs than a wavefront's LDS holds: counted, now with room in HBM
        unsigned long long w[SMC_WORDS];
        HIPCHECK(hipMemcpyAsync(w, a.out, sizeof w, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        ctx->sumLastBig = (u32)w[SMC_NFLAG];
        if (!w[SMC_NFLAG]) return GX_OK;
        flags.resize(nPk);
        HIPCHECK(hipMemcpyAsync(flags.data(), a.flag, nPk * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        big.clear();
        u64 runs = 0, blocks = 0;
        for (size_t k = 0; k < nPk; k++)
          if (flags[k]) {
            big.push_back(SumBig{(u32)k, flags[k], runs, 2 * blocks});
            runs += flags[k];
            blocks += (flags[k] + SUM_BLK - 1) / SUM_BLK;
          }
        if (big.size() != w[SMC_NFLAG] || runs != w[SMC_FLAGRUNS]) {
          ctx->err = "peak summits: the flagged peaks are not the ones counted";
          return GX_ERR_DEVICE;
        }
        POOLED(ctx, ctx->sumBig, big.size() * sizeof(SumBig));
        POOLED(ctx, ctx->sumScrStart, (size_t)runs * 4);
        POOLED(ctx, ctx->sumScrVal, (size_t)runs * 8);
        POOLED(ctx, ctx->sumScrBlk, (size_t)blocks * 16);
        HIPCHECK(hipMemcpyAsync(ctx->sumBig.p, big.data(), big.size() * sizeof(SumBig), hipMemcpyHostToDevice, s));
        a.big = ctx->sumBig.as<SumBig>();
        a.nBig = (u32)big.size();
        a.scrStart = ctx->sumScrStart.as<u32>();
        a.scrVal = ctx->sumScrVal.as<long long>();
        a.scrBlk = ctx->sumScrBlk.as<long long>();
        const u32 grid2 = grid ? grid : std::max(1u, std::min((a.nBig + wpb - 1) / wpb, SUM_GRID));
        hipLaunchKernelGGL(k_summits<true>, dim3(grid2), dim3(SUM_NT), 0, s, a);
        if (int rc__ = dbg_sync(ctx, "k_summits<big>")) return rc__;
        HIPCHECK(hipGetLastError());
        return GX_OK;
      }))
    return rc;
  phase_end(ctx);
  ctx->sumLastReruns = list.reruns;
  // the records come in the order of the races: placed by peak (a counting sort), each peak's few by position
  const size_t n = (size_t)h[SMC_COUNT];
  std::vector<SumRec> rec(n);
  if (n) {
    HIPCHECK(hipMemcpyAsync(rec.data(), ctx->sumList.p, n * sizeof(SumRec), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
  std::vector<size_t> first(nPk + 1, 0);
  for (const SumRec& r : rec) {
    if (r.peak >= nPk) {
      ctx->err = "peak summits: a summit of a peak the list does not have";
      return GX_ERR_DEVICE;
    }
    first[r.peak + 1]++;
  }
  for (size_t k = 0; k < nPk; k++) first[k + 1] += first[k];
  std::vector<size_t> at(first.begin(), first.end() - 1);
  res.resize(n);
  for (const SumRec& r : rec) memcpy(&res[at[r.peak]++], &r, sizeof r);
  for (size_t k = 0; k < nPk; k++)
    if (first[k + 1] - first[k] > 1)
      std::sort(res.begin() + first[k], res.begin() + first[k + 1], [](const gx_summit& a, const gx_summit& b) { return a.pos < b.pos; });
  return GX_OK;
}

// The domain: the pooled depth stays below 2^31 at every base.  Fewer than 2^31 / 120 pooled events cannot reach it; with more,
// the samples' own maxima per peak (psig_pass) must add up to less.
int sum_domain(gx_ctx* ctx, const std::vector<KeptView>& views, const std::vector<PsigPeak>& pk) {
  u64 n = 0;
  for (const ViewSize& z : kept_sizes(views)) n += z.n;
  if (n < PSIG_MAX_EVENTS || pk.empty() || views.empty()) return GX_OK;
  if (int rc = psig_pass(ctx, views, pk.data(), pk.size(), 0, ctx->sumMaxHost)) return rc;
  const PsigRec* r = static_cast<const PsigRec*>(ctx->sumMaxHost.p);
  for (size_t k = 0; k < pk.size(); k++) {
    long long sum = 0;
    for (size_t v = 0; v < views.size(); v++) sum += std::max<long long>(0, r[v * pk.size() + k].max);
    if (sum >= (1ll << 31)) return refuse(ctx, "gx_peak_summits: the treatments' depths in a peak add up to 2^31 or more (beyond the pooled pileup's domain)");
  }
  return GX_OK;
}

// the kept treatments in the peaks gx_find_peaks left
int peak_summits_kept(gx_ctx* ctx, u32 pPct, u32 rPct) {
  const size_t nPk = ctx->nHostPeaks;
  const gx_peak* hp = static_cast<const gx_peak*>(ctx->hPeaks.p);
  std::vector<PsigPeak> pk(nPk);
  for (size_t k = 0; k < nPk; k++) pk[k] = PsigPeak{hp[k].chrom, hp[k].start, hp[k].end, hp[k].summit};
  std::vector<KeptView> views;
  for (const gx_ctx::KeptSample& k : ctx->kept)
    if (!k.ctrl) views.push_back({&k.segs, &k.save});
  if (int rc = sum_domain(ctx, views, pk)) return rc;
  if (int rc = sum_pass(ctx, views, pk.data(), nPk, pPct, rPct, 0, 0, 0, ctx->sumRes)) return rc;
  ctx->sumReady = true;
  return GX_OK;
}

// a caller's host events as one sample whose save mask lists every chromosome, in the caller's peaks
int peak_summits_events(gx_ctx* ctx, const gx_event* ev, size_t n, const gx_region* peaks, size_t nPk, u32 pPct, u32 rPct, u32 grid, u32 runCap, u64 listCap,
                        std::vector<gx_summit>& res) {
  if (pPct > 100 || rPct > 100) return refuse(ctx, "gx_peak_summits_events: a percentage above 100");
  if ((u64)n >= PSIG_MAX_EVENTS) return refuse(ctx, "gx_peak_summits_events: 2^31 / 120 events or more (a depth of 2^31 is beyond the pileup's domain)");
  if (grid > 65535u) return refuse(ctx, "gx_peak_summits_events: more than 65535 workgroups");
  if (listCap >> 32) return refuse(ctx, "gx_peak_summits_events: a list of 2^32 entries or more");
  if (int rc = psig_check_peaks(ctx, peaks, nPk, nullptr, "gx_peak_summits_events")) return rc;
  std::vector<gx_ctx::Seg> segs;
  if (int rc = kept_upload(ctx, ev, n, false, segs)) return rc;
  std::vector<PsigPeak> pk(nPk);
  for (size_t k = 0; k < nPk; k++) pk[k] = PsigPeak{peaks[k].chrom, peaks[k].start, peaks[k].end, 0u};
  const int rc = sum_pass(ctx, {KeptView{&segs, nullptr}}, pk.data(), nPk, pPct, rPct, grid, runCap, listCap, res);
  if (n) (void)hipStreamSynchronize(ctx->stream);   // (the events are the caller's: a pass without peaks launches nothing)
  return rc;
}

}  // namespace
