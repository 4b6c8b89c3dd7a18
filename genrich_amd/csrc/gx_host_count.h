// gx_host_count.h -- the host side of gx_count_in_peaks (gx_count.h): which events each sample keeps, and the one count pass.
// (a part of gx_api.hip's translation unit)
#pragma once
namespace {

// gx_sample_end, counting on: the sample's pieces stay where its build read them.  The library's own buffers behind them (device
// chunks of host pushes, 16-byte copies of packed pieces, the survivors of the int16 rule) leave the context, which takes others
// for the next sample; a caller's device buffer is read in place (the caller keeps it, include/genrich_amd.h).
void keep_sample(gx_ctx* ctx, int isCtrl) {
  gx_ctx::KeptSample k;
  k.rep = ctx->sample;
  k.ctrl = isCtrl != 0;
  k.save = ctx->save;
  for (const gx_ctx::Seg& sg : ctx->segs)
    if (sg.n) k.segs.push_back({sg.p, sg.n, nullptr, sg.packed});   // (uploads: the build waited for them on the stream)
  const size_t used = std::min(ctx->evChunks.size(), ctx->evChunkIdx + (ctx->evChunkFill ? 1 : 0));
  for (size_t i = 0; i < used; i++) k.chunks.push_back(std::move(ctx->evChunks[i]));
  ctx->evChunks.erase(ctx->evChunks.begin(), ctx->evChunks.begin() + used);
  const size_t up = std::min(ctx->unpackBufs.size(), ctx->unpackUsed);
  for (size_t i = 0; i < up; i++) k.unpacks.push_back(std::move(ctx->unpackBufs[i]));
  ctx->unpackBufs.erase(ctx->unpackBufs.begin(), ctx->unpackBufs.begin() + up);
  if (ctx->satDone) k.sat = std::move(ctx->satBuf);
  ctx->evChunkIdx = ctx->evChunkFill = 0;
  ctx->unpackUsed = 0;
  ctx->kept.push_back(std::move(k));
}

// gx_reset / counting switched off: the kept buffers go back to the context (no free, no allocation in the next run)
void drop_kept(gx_ctx* ctx) {
  for (gx_ctx::KeptSample& k : ctx->kept) {
    for (DevBuf& b : k.chunks) ctx->evChunks.push_back(std::move(b));
    for (DevBuf& b : k.unpacks) ctx->unpackBufs.push_back(std::move(b));
    recycle(ctx, k.sat);
  }
  ctx->kept.clear();
  ctx->countsReady = ctx->regionsReady = false;
}

// The staging the passes over the kept samples share (count_in_peaks, count_in_regions, the complexity pass): a sample's view of
// the chromosome table, and its pieces cut into chunks of CNT_CHUNK events.
// save: the chromosomes the sample's pileup took (null: every one)
void stage_chroms(const gx_ctx* ctx, const std::vector<uint8_t>* save, CntChrom* ch) {
  for (u32 c = 0; c < ctx->nChrom; c++) {
    const DChrom& d = ctx->hChrom[c];
    const bool act = !ctx->skip[c] && (!save || (*save)[c]) && ctx->owned[c] && d.tileBase != NULL_TILE;
    ch[c] = CntChrom{act ? (u64)d.tileBase << TB : 0ull, d.len, act ? 1u : 0u};
  }
}
size_t chunks_of(const std::vector<gx_ctx::Seg>& segs) {
  size_t c = 0;
  for (const gx_ctx::Seg& sg : segs) c += (sg.n + CNT_CHUNK - 1) / CNT_CHUNK;
  return c;
}
CntChunk* stage_chunks(const std::vector<gx_ctx::Seg>& segs, CntChunk* at) {
  for (const gx_ctx::Seg& sg : segs) {
    const size_t esz = sg.packed ? sizeof(gx_event8) : sizeof(gx_event);
    for (size_t o = 0; o < sg.n; o += CNT_CHUNK)
      *at++ = CntChunk{reinterpret_cast<const char*>(sg.p) + o * esz, (u32)std::min<size_t>(CNT_CHUNK, sg.n - o), sg.packed ? 1u : 0u};
  }
  return at;
}
// chunk0[k] = the first chunk of kept sample k (chunk0[nS] = all of them)
std::vector<size_t> kept_chunk_offsets(const gx_ctx* ctx) {
  std::vector<size_t> chunk0(ctx->kept.size() + 1, 0);
  for (size_t k = 0; k < ctx->kept.size(); k++) chunk0[k + 1] = chunk0[k] + chunks_of(ctx->kept[k].segs);
  return chunk0;
}
// ch[nS * nChrom], ck[chunk0[nS]]
void stage_kept(const gx_ctx* ctx, const std::vector<size_t>& chunk0, CntChrom* ch, CntChunk* ck) {
  for (size_t k = 0; k < ctx->kept.size(); k++) {
    stage_chroms(ctx, &ctx->kept[k].save, ch + k * ctx->nChrom);
    stage_chunks(ctx->kept[k].segs, ck + chunk0[k]);
  }
}

int count_in_peaks(gx_ctx* ctx) {
  hipStream_t s = ctx->stream;
  const u32 nS = (u32)ctx->kept.size(), nChrom = ctx->nChrom;
  const size_t nPk = ctx->nHostPeaks;
  if (nPk >= 0xFFFFFFF0ull) {
    ctx->err = "too many peaks to count in";
    return GX_ERR_MEM;
  }
  const gx_peak* hp = static_cast<const gx_peak*>(ctx->hPeaks.p);
  // staging: the peaks in tile space (+ the sentinel), each sample's chromosome table, each sample's chunks
  const std::vector<size_t> chunk0 = kept_chunk_offsets(ctx);
  const size_t pkBytes = (nPk + 1) * sizeof(CntPeak), chBytes = (size_t)nS * nChrom * sizeof(CntChrom),
               ckBytes = chunk0[nS] * sizeof(CntChunk);
  const size_t total = pkBytes + chBytes + ckBytes;
  HIPCHECK(ctx->cntStage.ensure(total));
  HIPCHECK(ctx->cntIn.ensure(total));
  char* st = static_cast<char*>(ctx->cntStage.p);
  CntPeak* pk = reinterpret_cast<CntPeak*>(st);
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
  CntChrom* ch = reinterpret_cast<CntChrom*>(st + pkBytes);
  CntChunk* ck = reinterpret_cast<CntChunk*>(st + pkBytes + chBytes);
  stage_kept(ctx, chunk0, ch, ck);
  phase_begin(ctx, "count");
  HIPCHECK(hipMemcpyAsync(ctx->cntIn.p, st, total, hipMemcpyHostToDevice, s));
  const CntPeak* dPk = ctx->cntIn.as<CntPeak>();
  const CntChrom* dCh = reinterpret_cast<const CntChrom*>(ctx->cntIn.as<char>() + pkBytes);
  const CntChunk* dCk = reinterpret_cast<const CntChunk*>(ctx->cntIn.as<char>() + pkBytes + chBytes);
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
      // two workgroups per CU when the window leaves room for them; enough workgroups that none sees more than CNT_WG_CHUNKS chunks
      u32 grid = (u32)ctx->numCU * (a.wn * 4 <= 64 * 1024 ? 2u : 1u);
      grid = std::max(std::min(grid, nCk), (nCk + CNT_WG_CHUNKS - 1) / CNT_WG_CHUNKS);
      hipLaunchKernelGGL(k_cnt_count, dim3(grid), dim3(CNT_NT), (size_t)a.wn * 4, s, a);
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
