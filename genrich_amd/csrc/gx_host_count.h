// gx_host_count.h -- the host side of gx_count_in_peaks (gx_count.h): the peaks in tile space in front of the kept samples' views
// (gx_host_kept.h), the index, the windows of counters per sample, the scan.
// (a part of gx_api.hip's translation unit)
#pragma once
namespace {

int count_in_peaks(gx_ctx* ctx) {
  hipStream_t s = ctx->stream;
  const u32 nS = (u32)ctx->kept.size(), nChrom = ctx->nChrom;
  const size_t nPk = ctx->nHostPeaks;
  if (nPk >= 0xFFFFFFF0ull) {
    ctx->err = "too many peaks to count in";
    return GX_ERR_MEM;
  }
  const gx_peak* hp = static_cast<const gx_peak*>(ctx->hPeaks.p);
  // staging: the peaks in tile space (+ the sentinel) in front of the kept samples' views and chunks
  KeptIn in;
  if (int rc = kept_stage(ctx, kept_views(ctx), (nPk + 1) * sizeof(CntPeak), true, false, in)) return rc;
  const std::vector<size_t>& chunk0 = in.chunk0;
  CntPeak* pk = reinterpret_cast<CntPeak*>(in.front);
  for (size_t k = 0; k < nPk; k++) {
    const gx_peak& p = hp[k];
    if (p.chrom >= nChrom || ctx->hChrom[p.chrom].tileBase == NULL_TILE) {
      ctx->err = "a peak on a chromosome this context does not work on";
      return GX_ERR_DEVICE;
    }
    const u64 base = (u64)ctx->hChrom[p.chrom].tileBase << TB;
    pk[k] = CntPeak{base + p.start, base + p.end};
  }
  pk[nPk] = CntPeak{~0ull, ~0ull};
  phase_begin(ctx, "count");
  if (int rc = kept_send(ctx, in)) return rc;
  const CntPeak* dPk = reinterpret_cast<const CntPeak*>(in.dFront);
  const CntChrom* dCh = in.dCh;
  const CntChunk* dCk = in.dCk;
  // tile index, difference arrays, results ({counts, total, in_peaks} per sample)
  const u32 nIdx = ctx->nTiles + 1;
  HIPCHECK(ctx->cntIdx.ensure((size_t)nIdx * 8));
  const size_t stride = nPk + 2;
  HIPCHECK(ctx->cntDiff.ensure(std::max<size_t>(1, nS) * (nPk + 1) * 8));
  HIPCHECK(ctx->cntRes.ensure(std::max<size_t>(1, nS) * stride * 8));
  HIPCHECK(ctx->cntHost.ensure(std::max<size_t>(1, nS) * stride * 8));
  HIPCHECK(hipMemsetAsync(ctx->cntDiff.p, 0, (size_t)nS * (nPk + 1) * 8, s));
  HIPCHECK(hipMemsetAsync(ctx->cntRes.p, 0, (size_t)nS * stride * 8, s));
  u32* idx0 = ctx->cntIdx.as<u32>();
  u32* idx1 = idx0 + nIdx;
  hipLaunchKernelGGL(k_cnt_index, dim3(std::max(1u, std::min((nIdx + 255) / 256, (u32)(8 * ctx->numCU)))), dim3(256), 0, s, dPk, (u32)nPk,
                     nIdx, idx0, idx1);
  if (int rc__ = dbg_sync(ctx, "k_cnt_index")) return rc__;
  if (!ctx->cntLdsSet) {
    HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_cnt_count), hipFuncAttributeMaxDynamicSharedMemorySize, CNT_LDS_MAX * 4));
    ctx->cntLdsSet = true;
  }
  const size_t nDiff = nPk + 1;
  const u32 nWin = (u32)((nDiff + CNT_LDS_MAX - 1) / CNT_LDS_MAX);
  for (u32 k = 0; k < nS; k++) {
    const u32 nCk = (u32)(chunk0[k + 1] - chunk0[k]);
    if (!nCk) continue;
    for (u32 wdw = 0; wdw < nWin; wdw++) {
      CntArgs a;
      a.chunks = dCk + chunk0[k];
      a.nChunks = nCk;
      a.chroms = dCh + (size_t)k * nChrom;
      a.nChrom = nChrom;
      a.pk = dPk;
      a.idx0 = idx0;
      a.idx1 = idx1;
      a.w0 = wdw * CNT_LDS_MAX;
      a.wn = (u32)std::min<size_t>(CNT_LDS_MAX, nDiff - a.w0);
      a.diff = ctx->cntDiff.as<unsigned long long>() + (size_t)k * nDiff;
      a.tot = wdw == 0 ? ctx->cntRes.as<unsigned long long>() + (size_t)k * stride + nPk : nullptr;
      hipLaunchKernelGGL(k_cnt_count, dim3(kept_window_grid(ctx, a.wn, nCk)), dim3(CNT_NT), (size_t)a.wn * 4, s, a);
      if (int rc__ = dbg_sync(ctx, "k_cnt_count")) return rc__;
    }
  }
  if (nS && nPk)
    hipLaunchKernelGGL(k_cnt_scan, dim3(nS), dim3(CNT_NT), 0, s, ctx->cntDiff.as<long long>(), (u32)nPk, stride, ctx->cntRes.as<long long>());
  HIPCHECK(hipGetLastError());
  phase_end(ctx);
  HIPCHECK(hipMemcpyAsync(ctx->cntHost.p, ctx->cntRes.p, (size_t)nS * stride * 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  ctx->cntPk = (u32)nPk;
  ctx->countsReady = true;
  return GX_OK;
}

}  // namespace
