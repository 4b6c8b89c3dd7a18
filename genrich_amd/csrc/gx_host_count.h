// gx_host_count.h -- the kept samples on the host: which events each sample keeps (keep_sample), what every pass over them
// stages for the device (kept_stage; the passes: count_in_peaks here, gx_host_regions.h, gx_host_complexity.h,
// gx_host_subsample.h), and the host side of gx_count_in_peaks (gx_count.h).
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

// What a pass over kept events stages for the device (gx_kept.h), in ONE pinned area and ONE device buffer (ctx->keptStage,
// ctx->keptIn) that all the passes share -- each drains the stream before it returns:
//   front   the pass's own inputs, `front` bytes it fills itself between kept_stage and kept_send
//   dCh     [views][nChrom]  on request: each view's CntChrom table
//   dCk     [chunk0[views]]  each view's pieces cut into chunks of CNT_CHUNK events; view v's from chunk0[v] on
//   dFirst  [chunk0[views]]  on request: the view's events before each of its chunks
// A view is a sample's pieces and the chromosomes its pileup took (null: every one).
struct KeptView { const std::vector<gx_ctx::Seg>* segs; const std::vector<uint8_t>* save; };
struct KeptIn {
  char* front = nullptr;          // on the host
  const char* dFront = nullptr;   // ... and on the device, like the rest
  const CntChrom* dCh = nullptr;
  const CntChunk* dCk = nullptr;
  const u64* dFirst = nullptr;
  std::vector<size_t> chunk0;
  size_t bytes = 0;
};
std::vector<KeptView> kept_views(const gx_ctx* ctx) {
  std::vector<KeptView> v;
  for (const gx_ctx::KeptSample& k : ctx->kept) v.push_back({&k.segs, &k.save});
  return v;
}
int kept_stage(gx_ctx* ctx, const std::vector<KeptView>& views, size_t front, bool wantChroms, bool wantFirst, KeptIn& in) {
  const u32 nChrom = ctx->nChrom;
  in.chunk0.assign(views.size() + 1, 0);
  for (size_t v = 0; v < views.size(); v++) {
    size_t c = 0;
    for (const gx_ctx::Seg& sg : *views[v].segs) c += (sg.n + CNT_CHUNK - 1) / CNT_CHUNK;
    in.chunk0[v + 1] = in.chunk0[v] + c;
  }
  const size_t nCk = in.chunk0.back(), chAt = (front + 15) & ~(size_t)15, ckAt = chAt + (wantChroms ? views.size() * nChrom * sizeof(CntChrom) : 0),
               firstAt = ckAt + nCk * sizeof(CntChunk);
  in.bytes = firstAt + (wantFirst ? nCk * 8 : 0);
  HIPCHECK(ctx->keptStage.ensure(in.bytes));
  POOLED(ctx, ctx->keptIn, in.bytes);
  in.front = static_cast<char*>(ctx->keptStage.p);
  CntChrom* ch = reinterpret_cast<CntChrom*>(in.front + chAt);
  CntChunk* ck = reinterpret_cast<CntChunk*>(in.front + ckAt);
  u64* first = reinterpret_cast<u64*>(in.front + firstAt);
  for (const KeptView& view : views) {
    for (u32 c = 0; wantChroms && c < nChrom; c++) {
      const DChrom& d = ctx->hChrom[c];
      const bool act = !ctx->skip[c] && (!view.save || (*view.save)[c]) && ctx->owned[c] && d.tileBase != NULL_TILE;
      *ch++ = CntChrom{act ? (u64)d.tileBase << TB : 0ull, d.len, act ? 1u : 0u};
    }
    u64 run = 0;
    for (const gx_ctx::Seg& sg : *view.segs) {
      const size_t esz = sg.packed ? sizeof(gx_event8) : sizeof(gx_event);
      for (size_t o = 0; o < sg.n; o += CNT_CHUNK) {
        *ck = CntChunk{reinterpret_cast<const char*>(sg.p) + o * esz, (u32)std::min<size_t>(CNT_CHUNK, sg.n - o), sg.packed ? 1u : 0u};
        if (wantFirst) *first++ = run;
        run += (ck++)->n;
      }
    }
  }
  in.dFront = ctx->keptIn.as<char>();
  in.dCh = wantChroms ? reinterpret_cast<const CntChrom*>(in.dFront + chAt) : nullptr;
  in.dCk = reinterpret_cast<const CntChunk*>(in.dFront + ckAt);
  in.dFirst = wantFirst ? reinterpret_cast<const u64*>(in.dFront + firstAt) : nullptr;
  return GX_OK;
}
// the pass's one copy of its inputs
int kept_send(gx_ctx* ctx, const KeptIn& in) {
  HIPCHECK(hipMemcpyAsync(ctx->keptIn.p, ctx->keptStage.p, in.bytes, hipMemcpyHostToDevice, ctx->stream));
  return GX_OK;
}

// the grid of a launch with an LDS window of wn counters over nCk chunks (k_cnt_count, k_reg_count<true>): two workgroups per
// CU when the window leaves room for them; enough workgroups that none sees more than CNT_WG_CHUNKS chunks
u32 kept_window_grid(const gx_ctx* ctx, u32 wn, u32 nCk) {
  const u32 grid = (u32)ctx->numCU * (wn * 4 <= 64 * 1024 ? 2u : 1u);
  return std::max(std::min(grid, nCk), (nCk + CNT_WG_CHUNKS - 1) / CNT_WG_CHUNKS);
}

// a sample's counted row {count[n], total, in} to the caller (gx_get_peak_counts, gx_get_region_counts): min(cap, n) counts
int give_counts(const gx_ctx* ctx, const PinnedBuf& host, size_t n, int sample, int* rep, int* is_ctrl, int64_t* count120, size_t cap,
                int64_t* total120, int64_t* in120) {
  const int64_t* r = static_cast<const int64_t*>(host.p) + (size_t)sample * (n + 2);
  if (rep) *rep = ctx->kept[sample].rep;
  if (is_ctrl) *is_ctrl = ctx->kept[sample].ctrl ? 1 : 0;
  if (const size_t k = std::min(cap, n)) memcpy(count120, r, k * sizeof(int64_t));
  if (total120) *total120 = r[n];
  if (in120) *in120 = r[n + 1];
  return GX_OK;
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
