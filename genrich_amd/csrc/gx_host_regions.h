// gx_host_regions.h -- the host side of gx_count_in_regions (gx_regions.h): the regions put into tile space and ranked, the
// count pass over the kept samples (gx_host_kept.h keep_sample), the scans, the gather and the inverted intervals.
// (a part of gx_api.hip's translation unit)
#pragma once
namespace {

// key[0 .. m) of the live regions in input order, rank[k] = region k's place in it (~0: not live) -> the keys sorted, the
// ranks following them (ties in any order)
void rank_regions(u64* key, u32 m, u32* rank, size_t n) {
  std::vector<std::pair<u64, u32>> v(m);
  for (u32 i = 0; i < m; i++) v[i] = {key[i], i};
  std::sort(v.begin(), v.end());
  std::vector<u32> place(m);
  for (u32 i = 0; i < m; i++) {
    key[i] = v[i].first;
    place[v[i].second] = i;
  }
  for (size_t k = 0; k < n; k++)
    if (rank[k] != ~0u) rank[k] = place[rank[k]];
}

int count_in_regions(gx_ctx* ctx, const gx_region* reg, size_t n) {
  hipStream_t s = ctx->stream;
  const u32 nS = (u32)ctx->kept.size(), nChrom = ctx->nChrom;
  if (n >= 0x7FFFFFF0ull) {
    ctx->err = "too many regions to count in";
    return GX_ERR_MEM;
  }
  const size_t stride = n + 2;   // per sample: the counts, total, in_regions
  HIPCHECK(ctx->regHost.ensure(std::max<size_t>(1, nS) * stride * 8));
  ctx->regN = n;
  ctx->regSamples = nS;
  if (!nS) return GX_OK;
  // staging: A, B (room for n + a sentinel each) and the regions' ranks in front of the kept samples' views and chunks
  const size_t abBytes = (n + 1) * 8, rkBytes = ((n + 1) & ~(size_t)1) * 4;
  KeptIn in;
  if (int rc = kept_stage(ctx, kept_views(ctx), 2 * abBytes + 2 * rkBytes, true, false, in)) return rc;
  const std::vector<size_t>& chunk0 = in.chunk0;
  char* st = in.front;
  u64* hA = reinterpret_cast<u64*>(st);
  u64* hB = reinterpret_cast<u64*>(st + abBytes);
  u32* hRa = reinterpret_cast<u32*>(st + 2 * abBytes);
  u32* hRb = reinterpret_cast<u32*>(st + 2 * abBytes + rkBytes);
  // the live regions in tile space; a BED file is usually sorted, and then its starts (and often its ends) are A (and B) as they come
  u32 m = 0;
  bool sortedA = true, sortedB = true;
  for (size_t k = 0; k < n; k++) {
    const gx_region& r = reg[k];
    hRa[k] = hRb[k] = ~0u;
    if (r.chrom >= nChrom) continue;
    const DChrom& d = ctx->hChrom[r.chrom];
    if (ctx->skip[r.chrom] || !ctx->owned[r.chrom] || d.tileBase == NULL_TILE || r.start >= d.len) continue;
    const u64 base = (u64)d.tileBase << TB;
    hA[m] = base + r.start;
    hB[m] = base + std::min(r.end, d.len);
    sortedA = sortedA && (m == 0 || hA[m - 1] <= hA[m]);
    sortedB = sortedB && (m == 0 || hB[m - 1] <= hB[m]);
    hRa[k] = hRb[k] = m++;
  }
  if (!sortedA) rank_regions(hA, m, hRa, n);
  if (!sortedB) rank_regions(hB, m, hRb, n);
  hA[m] = hB[m] = ~0ull;
  const char* din = in.dFront;
  const u64* dA = reinterpret_cast<const u64*>(din);
  const u64* dB = reinterpret_cast<const u64*>(din + abBytes);
  const u32* dRa = reinterpret_cast<const u32*>(din + 2 * abBytes);
  const u32* dRb = reinterpret_cast<const u32*>(din + 2 * abBytes + rkBytes);
  const CntChrom* dCh = in.dCh;
  const CntChunk* dCk = in.dCk;
  // tile index, histograms, tile sums of the scans, results, the inverted intervals' list (+ its counter)
  const u32 nIdx = ctx->nTiles + 1;
  const size_t seg = (size_t)m + 1, nH = 2 * seg;
  const u32 nT = (m + REG_SCAN_TILE - 1) / REG_SCAN_TILE;
  const u32 nWin = (u32)((nH + CNT_LDS_MAX - 1) / CNT_LDS_MAX);
  const int winMax = ctx->knob.regWindows ? ctx->knob.regWindows : (int)REG_WIN_MAX;   // (GX_REG_WINDOWS: < 0 = never in LDS)
  const bool lds = (int)nWin <= winMax;
  HIPCHECK(ctx->regIdx.ensure((size_t)nIdx * sizeof(uint4)));
  HIPCHECK(ctx->regHist.ensure((size_t)nS * nH * 8));
  HIPCHECK(ctx->regSums.ensure((size_t)2 * nS * (nT + 1) * 8 * 2));
  HIPCHECK(ctx->regRes.ensure((size_t)nS * stride * 8));
  uint4* idx = ctx->regIdx.as<uint4>();
  long long* sums = ctx->regSums.as<long long>();
  long long* pre = sums + (size_t)2 * nS * (nT + 1);
  if (!ctx->regLdsSet) {
    HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_reg_count<true>), hipFuncAttributeMaxDynamicSharedMemorySize, CNT_LDS_MAX * 4));
    ctx->regLdsSet = true;
  }
  phase_begin(ctx, "regions");
  if (int rc = kept_send(ctx, in)) return rc;
  hipLaunchKernelGGL(k_reg_index, dim3(std::max(1u, std::min((nIdx + 255) / 256, (u32)(8 * ctx->numCU)))), dim3(256), 0, s, dA, dB, m, nIdx,
                     idx);
  if (int rc__ = dbg_sync(ctx, "k_reg_index")) return rc__;
  for (;;) {   // (again only when more inverted intervals turned up than the list holds)
    const u32 invCap = ctx->regInvCap;
    HIPCHECK(ctx->regInv.ensure((size_t)invCap * sizeof(RegInv) + 8));
    RegInv* dInv = ctx->regInv.as<RegInv>();
    u32* dNInv = reinterpret_cast<u32*>(ctx->regInv.as<char>() + (size_t)invCap * sizeof(RegInv));
    HIPCHECK(hipMemsetAsync(dNInv, 0, 8, s));
    HIPCHECK(hipMemsetAsync(ctx->regHist.p, 0, (size_t)nS * nH * 8, s));
    HIPCHECK(hipMemsetAsync(ctx->regRes.p, 0, (size_t)nS * stride * 8, s));
    for (u32 k = 0; k < nS; k++) {
      const u32 nCk = (u32)(chunk0[k + 1] - chunk0[k]);
      if (!nCk) continue;
      RegArgs a;
      a.chunks = dCk + chunk0[k];
      a.nChunks = nCk;
      a.chroms = dCh + (size_t)k * nChrom;
      a.nChrom = nChrom;
      a.A = dA;
      a.B = dB;
      a.idx = idx;
      a.m = m;
      a.hist = ctx->regHist.as<unsigned long long>() + (size_t)k * nH;
      a.inv = dInv;
      a.nInv = dNInv;
      a.invCap = invCap;
      a.sample = k;
      unsigned long long* tot = ctx->regRes.as<unsigned long long>() + (size_t)k * stride + n;
      if (!lds) {
        a.w0 = 0;
        a.wn = 0;
        a.tot = tot;
        hipLaunchKernelGGL(k_reg_count<false>, dim3(std::max(1u, std::min(2u * (u32)ctx->numCU, nCk))), dim3(CNT_NT), 0, s, a);
        if (int rc__ = dbg_sync(ctx, "k_reg_count<global>")) return rc__;
        continue;
      }
      for (u32 wdw = 0; wdw < nWin; wdw++) {
        a.w0 = wdw * CNT_LDS_MAX;
        a.wn = (u32)std::min<size_t>(CNT_LDS_MAX, nH - a.w0);
        a.tot = wdw == 0 ? tot : nullptr;
        hipLaunchKernelGGL(k_reg_count<true>, dim3(kept_window_grid(ctx, a.wn, nCk)), dim3(CNT_NT), (size_t)a.wn * 4, s, a);
        if (int rc__ = dbg_sync(ctx, "k_reg_count<lds>")) return rc__;
      }
    }
    if (m) {
      long long* H = ctx->regHist.as<long long>();
      hipLaunchKernelGGL(k_reg_tile_sums, dim3(nT, 2 * nS), dim3(CNT_NT), 0, s, H, m, seg, nT, sums);
      hipLaunchKernelGGL(k_cnt_scan, dim3(2 * nS), dim3(CNT_NT), 0, s, sums, nT, (size_t)nT + 1, pre);
      hipLaunchKernelGGL(k_reg_tile_scan, dim3(nT, 2 * nS), dim3(CNT_NT), 0, s, H, m, seg, nT, pre);
      if (int rc__ = dbg_sync(ctx, "k_reg_tile_scan")) return rc__;
      hipLaunchKernelGGL(k_reg_gather, dim3(std::max(1u, std::min((u32)((n + 255) / 256), (u32)(8 * ctx->numCU))), nS), dim3(256), 0, s, H, m, dRa,
                         dRb, (u32)n, stride, ctx->regRes.as<long long>());
      hipLaunchKernelGGL(k_reg_inverted, dim3(std::max(1, ctx->numCU)), dim3(CNT_NT), 0, s, dInv, dNInv, invCap, dA, dB, dRa, dRb, (u32)n, stride,
                         ctx->regRes.as<unsigned long long>());
      if (int rc__ = dbg_sync(ctx, "k_reg_inverted")) return rc__;
    }
    HIPCHECK(hipGetLastError());
    phase_end(ctx);
    u32* hNInv = reinterpret_cast<u32*>(st);   // (the staging area has been sent: its front, A's 8 bytes at least, is free)
    HIPCHECK(hipMemcpyAsync(ctx->regHost.p, ctx->regRes.p, (size_t)nS * stride * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(hNInv, dNInv, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (*hNInv <= invCap) break;
    ctx->regInvCap = *hNInv + *hNInv / 2;
  }
  return GX_OK;
}

}  // namespace
