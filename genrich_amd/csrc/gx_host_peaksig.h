// gx_host_peaksig.h -- the host side of gx_peak_signal (gx_peaksig.h): the peaks put into tile space and into peak space, the
// two kernels per sample over one reused buffer, the one read-back; the pass over the kept samples and the one over a
// caller's events and peaks.
// (a part of gx_api.hip's translation unit)
#pragma once
namespace {

struct PsigPeak { u32 chrom, start, end, summit; };   // summit: from start

constexpr u64 PSIG_MAX_EVENTS = ((u64)1 << 31) / 120;   // gx_peak_signal_events: as many unit intervals on one base reach 2^31

// What a pass over the peak space stages (psig_pass, gx_host_summits.h): the peaks pkv[nPk] (sorted, disjoint, on chromosomes
// this context works on) in tile space with their sentinel, their first slots and their summit bases in front of the views and
// chunks; the tile index (the count's) and the peak space itself.  The phase `phase` is open when it returns GX_OK.
struct PsigStaged {
  KeptIn in;
  const CntPeak* dPk = nullptr;
  const u64* dOff = nullptr;
  const u32* dSum = nullptr;
  u32* idx0 = nullptr;
  u64 slots = 0;
};
int psig_stage(gx_ctx* ctx, const std::vector<KeptView>& views, const PsigPeak* pkv, size_t nPk, const char* phase, PsigStaged& st) {
  hipStream_t s = ctx->stream;
  const u32 nChrom = ctx->nChrom;
  KeptIn& in = st.in;
  const size_t pkBytes = (nPk + 1) * sizeof(CntPeak), offBytes = (nPk + 1) * 8, sumBytes = (nPk * 4 + 15) & ~(size_t)15;
  if (int rc = kept_stage(ctx, views, pkBytes + offBytes + sumBytes, true, false, in)) return rc;
  CntPeak* pk = reinterpret_cast<CntPeak*>(in.front);
  u64* off = reinterpret_cast<u64*>(in.front + pkBytes);
  u32* sum = reinterpret_cast<u32*>(in.front + pkBytes + offBytes);
  u64 slots = 0;
  for (size_t k = 0; k < nPk; k++) {
    const PsigPeak& p = pkv[k];
    if (p.chrom >= nChrom || ctx->hChrom[p.chrom].tileBase == NULL_TILE) {
      ctx->err = "a peak on a chromosome this context does not work on";
      return GX_ERR_DEVICE;
    }
    const u64 base = (u64)ctx->hChrom[p.chrom].tileBase << TB;
    pk[k] = CntPeak{base + p.start, base + p.end};
    off[k] = slots;
    sum[k] = p.summit;
    slots += ((u64)(p.end - p.start) + PSIG_PAD - 1) / PSIG_PAD * PSIG_PAD;
  }
  pk[nPk] = CntPeak{~0ull, ~0ull};
  off[nPk] = slots;
  st.slots = slots;
  st.dPk = reinterpret_cast<const CntPeak*>(in.dFront);
  st.dOff = reinterpret_cast<const u64*>(in.dFront + pkBytes);
  st.dSum = reinterpret_cast<const u32*>(in.dFront + pkBytes + offBytes);
  const u32 nIdx = ctx->nTiles + 1;
  HIPCHECK(ctx->cntIdx.ensure((size_t)nIdx * 8));
  POOLED(ctx, ctx->psigSpace, (size_t)slots * 4);
  st.idx0 = ctx->cntIdx.as<u32>();
  phase_begin(ctx, phase);
  if (int rc = kept_send(ctx, in)) return rc;
  hipLaunchKernelGGL(k_cnt_index, dim3(std::max(1u, std::min((nIdx + 255) / 256, (u32)(8 * ctx->numCU)))), dim3(256), 0, s, st.dPk, (u32)nPk,
                     nIdx, st.idx0, st.idx0 + nIdx);
  return dbg_sync(ctx, "k_cnt_index");
}
// view k's difference array added into the peak space (the caller clears it)
int psig_scatter(gx_ctx* ctx, const PsigStaged& st, u32 k, u32 grid) {
  const KeptIn& in = st.in;
  const u32 nCk = (u32)(in.chunk0[k + 1] - in.chunk0[k]);
  if (!nCk) return GX_OK;
  PsigArgs a;
  a.chunks = in.dCk + in.chunk0[k];
  a.nChunks = nCk;
  a.chroms = in.dCh + (size_t)k * ctx->nChrom;
  a.nChrom = ctx->nChrom;
  a.pk = st.dPk;
  a.idx0 = st.idx0;
  a.off = st.dOff;
  a.space = ctx->psigSpace.as<int>();
  hipLaunchKernelGGL(k_psig_scatter, dim3(grid ? grid : std::max(1u, std::min(2u * (u32)ctx->numCU, nCk))), dim3(CNT_NT), 0, ctx->stream, a);
  return dbg_sync(ctx, "k_psig_scatter");
}

// the views' depth in the peaks pkv[nPk] -> host[view][peak].
// grid = 0: the library's geometry, else that many workgroups for either kernel.
int psig_pass(gx_ctx* ctx, const std::vector<KeptView>& views, const PsigPeak* pkv, size_t nPk, u32 grid, PinnedBuf& host) {
  hipStream_t s = ctx->stream;
  const u32 nS = (u32)views.size();
  if (nPk >= 0xFFFFFFF0ull) {
    ctx->err = "too many peaks to take the signal in";
    return GX_ERR_MEM;
  }
  HIPCHECK(host.ensure(std::max<size_t>(1, (size_t)nS * nPk) * sizeof(PsigRec)));
  if (!nS || !nPk) return GX_OK;
  POOLED(ctx, ctx->psigRes, (size_t)nS * nPk * sizeof(PsigRec));
  PsigStaged st;
  if (int rc = psig_stage(ctx, views, pkv, nPk, "peaksig", st)) return rc;
  const u64 slots = st.slots;
  const CntPeak* dPk = st.dPk;
  const u64* dOff = st.dOff;
  const u32* dSum = st.dSum;
  PsigRec* res = ctx->psigRes.as<PsigRec>();
  const u32 rGrid = grid ? grid : std::max(1u, std::min((u32)((nPk + PSIG_NT / 64 - 1) / (PSIG_NT / 64)), PSIG_GRID));
  for (u32 k = 0; k < nS; k++) {
    HIPCHECK(hipMemsetAsync(ctx->psigSpace.p, 0, (size_t)slots * 4, s));
    if (int rc = psig_scatter(ctx, st, k, grid)) return rc;
    hipLaunchKernelGGL(k_psig_reduce, dim3(rGrid), dim3(PSIG_NT), 0, s, ctx->psigSpace.as<int>(), dOff, dPk, dSum, (u32)nPk, res + (size_t)k * nPk);
    if (int rc__ = dbg_sync(ctx, "k_psig_reduce")) return rc__;
  }
  HIPCHECK(hipGetLastError());
  phase_end(ctx);
  HIPCHECK(hipMemcpyAsync(host.p, res, (size_t)nS * nPk * sizeof(PsigRec), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return GX_OK;
}

// every kept sample in the peaks gx_find_peaks left
int peak_signal_kept(gx_ctx* ctx) {
  const size_t nPk = ctx->nHostPeaks;
  const gx_peak* hp = static_cast<const gx_peak*>(ctx->hPeaks.p);
  std::vector<PsigPeak> pk(nPk);
  for (size_t k = 0; k < nPk; k++) pk[k] = PsigPeak{hp[k].chrom, hp[k].start, hp[k].end, hp[k].summit};
  if (int rc = psig_pass(ctx, kept_views(ctx), pk.data(), nPk, 0, ctx->psigHost)) return rc;
  ctx->psigPk = nPk;
  ctx->psigReady = true;
  return GX_OK;
}

// what gx_peak_signal_events checks before anything is allocated or launched: the peaks sorted, disjoint, not empty, inside
// their chromosomes, which this context works on; the summit bases inside their peaks
int psig_check_peaks(gx_ctx* ctx, const gx_region* peaks, size_t nPk, const uint32_t* summitOff, const char* fn = "gx_peak_signal_events") {
  const std::string f(fn);
  for (size_t k = 0; k < nPk; k++) {
    const gx_region& r = peaks[k];
    if (r.chrom >= ctx->nChrom) return refuse(ctx, f + ": a peak on a chromosome the table does not have");
    if (r.start >= r.end || r.end > ctx->len[r.chrom]) return refuse(ctx, f + ": a peak that is empty or reaches beyond its chromosome");
    if (ctx->skip[r.chrom] || !ctx->owned[r.chrom] || ctx->hChrom[r.chrom].tileBase == NULL_TILE)
      return refuse(ctx, f + ": a peak on a chromosome this context does not work on");
    if (k && (peaks[k - 1].chrom > r.chrom || (peaks[k - 1].chrom == r.chrom && peaks[k - 1].end > r.start)))
      return refuse(ctx, f + ": the peaks are not sorted or overlap");
    if (summitOff && summitOff[k] >= r.end - r.start) return refuse(ctx, f + ": a summit outside its peak");
  }
  return GX_OK;
}

// a caller's host events as one sample whose save mask lists every chromosome, in the caller's peaks
int peak_signal_events(gx_ctx* ctx, const gx_event* ev, size_t n, const gx_region* peaks, size_t nPk, const uint32_t* summitOff, u32 grid) {
  if ((u64)n >= PSIG_MAX_EVENTS) return refuse(ctx, "gx_peak_signal_events: 2^31 / 120 events or more (a depth of 2^31 is beyond the pileup's domain)");
  if (grid > 65535u) return refuse(ctx, "gx_peak_signal_events: more than 65535 workgroups");
  if (int rc = psig_check_peaks(ctx, peaks, nPk, summitOff)) return rc;
  std::vector<gx_ctx::Seg> segs;
  if (int rc = kept_upload(ctx, ev, n, false, segs)) return rc;
  std::vector<PsigPeak> pk(nPk);
  for (size_t k = 0; k < nPk; k++) pk[k] = PsigPeak{peaks[k].chrom, peaks[k].start, peaks[k].end, summitOff ? summitOff[k] : 0u};
  const int rc = psig_pass(ctx, {KeptView{&segs, nullptr}}, pk.data(), nPk, grid, ctx->psigEvHost);
  if (n) (void)hipStreamSynchronize(ctx->stream);   // (the events are the caller's: a pass without peaks launches nothing)
  return rc;
}

// one view's records to the caller: min(cap, n) of each figure; any pointer may be NULL
void psig_give(const PsigRec* r, size_t n, size_t cap, int64_t* area120, int64_t* max120, uint32_t* summit, uint32_t* covered, int64_t* at120) {
  const size_t m = std::min(cap, n);
  for (size_t k = 0; k < m; k++) {
    if (area120) area120[k] = r[k].area;
    if (max120) max120[k] = r[k].max;
    if (summit) summit[k] = r[k].summit;
    if (covered) covered[k] = r[k].covered;
    if (at120) at120[k] = r[k].at;
  }
}

}  // namespace
