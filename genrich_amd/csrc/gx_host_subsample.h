// gx_host_subsample.h -- the host side of the subsample (gx_subsample.h) and of the peak saturation curve made with it
// (gx_saturation): the staging, the three launches, and the re-call of the peaks on a child context; then the split of a sample
// into both halves (k_sub_split) and the reproducibility calls made of the halves on the same child (gx_reproducibility).
// (a part of gx_api.hip's translation unit)
#pragma once
namespace {

// one sample's pieces -> its chunk list and the events before each chunk, on the device (gx_host_kept.h kept_stage); *n =
// its events
int sub_stage(gx_ctx* ctx, const std::vector<gx_ctx::Seg>& segs, const CntChunk** dCk, const u64** dFirst, u32* nCk, u64* n) {
  const ViewSize z = kept_sizes({KeptView{&segs, nullptr}})[0];
  const u64 nc = z.nCk;
  *n = z.n;
  *nCk = 0;
  if (nc > 0xFFFFFFFFull / SUB_BPC) return refuse(ctx, "subsample: a sample of 2^32 events or more");
  *nCk = (u32)nc;
  if (!nc) return GX_OK;
  KeptIn in;
  if (int rc = kept_stage(ctx, {KeptView{&segs, nullptr}}, 0, false, true, in)) return rc;
  if (int rc = kept_send(ctx, in)) return rc;
  HIPCHECK(hipStreamSynchronize(ctx->stream));   // (the pieces may be this call's)
  *dCk = in.dCk;
  *dFirst = in.dFirst;
  return GX_OK;
}

// the three launches over a staged sample of n events: the kept ones into `out` (at least n events), in order; *nKept of them.
// grid = 0: the library's choice.  The stream is drained before the return: `out` is ready for another stream.
int sub_pass(gx_ctx* ctx, const CntChunk* dCk, const u64* dFirst, u32 nCk, u64 n, u64 key, u64 T, u32 grid, DevBuf& out, u64* nKept) {
  *nKept = 0;
  if (!nCk || !n) return GX_OK;
  hipStream_t s = ctx->stream;
  const u32 nBlocks = nCk * SUB_BPC;
  POOLED(ctx, ctx->subCnt, (size_t)nBlocks * 4);
  POOLED(ctx, ctx->subOff, ((size_t)nBlocks + 1) * 8);
  POOLED(ctx, out, (size_t)n * sizeof(gx_event));
  SubArgs a;
  a.chunks = dCk;
  a.first = dFirst;
  a.nChunks = nCk;
  a.key = key;
  a.T = T;
  a.blockCnt = ctx->subCnt.as<u32>();
  a.blockOff = ctx->subOff.as<u64>();
  a.out = out.as<uint4>();
  const u32 g = grid ? grid : std::min(nBlocks, SUB_GRID);
  phase_begin(ctx, "subsample");
  hipLaunchKernelGGL(k_sub_count, dim3(g), dim3(SUB_NT), 0, s, a);
  if (int rc__ = dbg_sync(ctx, "k_sub_count")) return rc__;
  hipLaunchKernelGGL(k_sub_scan, dim3(1), dim3(SUB_SCAN_NT), 0, s, a.blockCnt, nBlocks, ctx->subOff.as<u64>());
  if (int rc__ = dbg_sync(ctx, "k_sub_scan")) return rc__;
  hipLaunchKernelGGL(k_sub_write, dim3(g), dim3(SUB_NT), 0, s, a);
  if (int rc__ = dbg_sync(ctx, "k_sub_write")) return rc__;
  phase_end(ctx);
  HIPCHECK(hipGetLastError());
  ctx->subUsed = true;
  u64 total = 0;
  HIPCHECK(hipMemcpyAsync(&total, ctx->subOff.as<u64>() + nBlocks, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (total > n) {
    ctx->err = "subsample: more events kept than there are";
    return GX_ERR_DEVICE;
  }
  *nKept = total;
  return GX_OK;
}

int sub_give(gx_ctx* ctx, const DevBuf& buf, u64 nKept, gx_event* out, size_t cap, size_t* n_out) {
  if (n_out) *n_out = (size_t)nKept;
  const size_t n = std::min<size_t>(cap, (size_t)nKept);
  if (n) {
    HIPCHECK(hipMemcpyAsync(out, buf.p, n * sizeof(gx_event), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
  }
  return GX_OK;
}

// kept sample k through the kernels, into its own buffer (ctx->subBufs[k])
int sub_kept(gx_ctx* ctx, size_t k, u64 seed, u64 T, u64* n, u64* nKept) {
  if (ctx->subBufs.size() < ctx->kept.size()) ctx->subBufs.resize(ctx->kept.size());
  const CntChunk* dCk = nullptr;
  const u64* dFirst = nullptr;
  u32 nCk = 0;
  if (int rc = sub_stage(ctx, ctx->kept[k].segs, &dCk, &dFirst, &nCk, n)) return rc;
  return sub_pass(ctx, dCk, dFirst, nCk, *n, subsample_key(seed, (u32)k), T, 0, ctx->subBufs[k], nKept);
}

void sat_drop(gx_ctx* ctx) {
  if (ctx->satChild) gx_destroy(ctx->satChild);
  ctx->satChild = nullptr;
  for (DevBuf& b : ctx->subBufs) recycle(ctx, b);
  ctx->subBufs.clear();
  ctx->satPts.clear();
  ctx->satPeaks.clear();
  ctx->subUsed = false;
}

// the child context the re-calls run on: the parent's device, parameters, chromosome table and switches; every extra off
int sat_child(gx_ctx* ctx) {
  if (!ctx->satChild) {
    gx_ctx* ch = nullptr;
    if (int rc = gx_create(&ch, &ctx->par)) {
      ctx->err = std::string("saturation: ") + (ch ? ch->err : std::string(gx_strerror(rc)));
      if (ch) gx_destroy(ch);
      return rc;
    }
    ctx->satChild = ch;
    ch->knob = ctx->knob;   // (GX_SBSHIFT is read when the tiles are laid out)
    std::vector<const uint32_t*> bed(ctx->nChrom, nullptr);
    std::vector<int32_t> bedLen(ctx->nChrom, 0);
    for (u32 c = 0; c < ctx->nChrom; c++) {
      bed[c] = ctx->bed[c].data();
      bedLen[c] = (int32_t)ctx->bed[c].size();
    }
    int rc = gx_set_chroms(ch, (int)ctx->nChrom, ctx->len.data(), ctx->skip.data(), bed.data(), bedLen.data());
    if (!rc && std::find(ctx->owned.begin(), ctx->owned.end(), 0) != ctx->owned.end()) rc = gx_set_owned(ch, ctx->owned.data());
    if (!rc) rc = gx_set_keep_pileups(ch, 0);
    if (rc) {
      ctx->err = "saturation: " + ch->err;
      gx_destroy(ch);
      ctx->satChild = nullptr;
      return rc;
    }
  }
  gx_ctx* ch = ctx->satChild;
  ch->par = ctx->par;
  ch->knob = ctx->knob;
  ch->forceColl = false;   // (one rank: the parent's is refused otherwise)
  ch->fracHint = ctx->fracHint;
  return GX_OK;
}

// a kept sample's pieces pushed whole into the child's open sample, read where they lie
int sat_push_whole(gx_ctx* ch, const gx_ctx::KeptSample& k) {
  for (const gx_ctx::Seg& sg : k.segs) {
    const int rc = sg.packed ? gx_push_events_packed(ch, reinterpret_cast<const gx_event8*>(sg.p), sg.n, GX_EVENTS_DEVICE)
                             : gx_push_events_device(ch, sg.p, sg.n);
    if (rc) return rc;
  }
  return GX_OK;
}

// one point: the run once more on the child, the treatments (with GX_SAT_CONTROLS the controls too) subsampled at T
int sat_point(gx_ctx* ctx, u64 T, u64 seed, unsigned flags, gx_sat_point& pt, std::vector<gx_peak>& peaks) {
  gx_ctx* ch = ctx->satChild;
  pt = gx_sat_point{};
  pt.threshold = T;
  peaks.clear();
  // every subsample first (each kept sample has a buffer of its own): n_total and n_kept cover all the subsampled samples,
  // also at a point whose re-call ends early
  const size_t nS = ctx->kept.size();
  std::vector<int> kt((size_t)ctx->sample, -1), kc((size_t)ctx->sample, -1);
  std::vector<u64> nk(nS, 0);
  for (size_t k = 0; k < nS; k++) {
    const gx_ctx::KeptSample& ks = ctx->kept[k];
    if (ks.rep < 0 || ks.rep >= ctx->sample) continue;
    (ks.ctrl ? kc : kt)[ks.rep] = (int)k;
    if (ks.ctrl && !(flags & GX_SAT_CONTROLS)) continue;
    u64 n = 0;
    if (int rc = sub_kept(ctx, k, seed, T, &n, &nk[k])) return rc;   // (the parent's own failure, with its own text)
    pt.n_total += n;
    pt.n_kept += nk[k];
  }
  int rc = gx_reset(ch);
  for (int r = 0; !rc && r < ctx->sample; r++) {
    if (kt[r] < 0) return refuse(ctx, "saturation: a replicate whose treatment was not kept");
    rc = gx_sample_begin(ch, 0, ctx->kept[kt[r]].save.data());
    if (!rc && nk[kt[r]]) rc = gx_push_events_device(ch, ctx->subBufs[kt[r]].as<gx_event>(), (size_t)nk[kt[r]]);
    if (!rc) rc = gx_sample_end(ch, nullptr, nullptr, nullptr);
    if (rc) break;
    if (kc[r] >= 0) {
      rc = gx_sample_begin(ch, 1, nullptr);
      if (!rc && (flags & GX_SAT_CONTROLS)) {
        if (nk[kc[r]]) rc = gx_push_events_device(ch, ctx->subBufs[kc[r]].as<gx_event>(), (size_t)nk[kc[r]]);
      } else if (!rc)
        rc = sat_push_whole(ch, ctx->kept[kc[r]]);
      if (!rc) rc = gx_sample_end(ch, nullptr, nullptr, nullptr);
    } else
      rc = gx_sample_no_control(ch, nullptr);
    if (!rc) rc = gx_pvalues(ch);
  }
  size_t np = 0;
  uint64_t g = 0, bp = 0;
  if (!rc) rc = gx_find_peaks(ch, &np, &g, &bp);
  if (rc == GX_ERR_EXPT) {   // (the subsample left no analyzable fragment: a result)
    pt.status = GX_ERR_EXPT;
    return GX_OK;
  }
  if (rc) {
    ctx->err = "saturation: " + ch->err;
    return rc;
  }
  pt.n_peaks = np;
  pt.peak_bp = bp;
  pt.genome_len = g;
  peaks.resize(np);
  if (np) rc = gx_get_peaks(ch, peaks.data(), np);
  return rc;
}

// ---- both halves of a sample (k_sub_split) and the reproducibility calls made of them (gx_reproducibility) ----

// sub_pass with k_sub_split as the third launch: all n events into `out`, half A in [0, *nA), half B behind it
int sub_split_pass(gx_ctx* ctx, const CntChunk* dCk, const u64* dFirst, u32 nCk, u64 n, u64 key, u64 T, u32 grid, DevBuf& out, u64* nA) {
  *nA = 0;
  if (!nCk || !n) return GX_OK;
  hipStream_t s = ctx->stream;
  const u32 nBlocks = nCk * SUB_BPC;
  POOLED(ctx, ctx->subCnt, (size_t)nBlocks * 4);
  POOLED(ctx, ctx->subOff, ((size_t)nBlocks + 1) * 8);
  POOLED(ctx, out, (size_t)n * sizeof(gx_event));
  SubArgs a;
  a.chunks = dCk;
  a.first = dFirst;
  a.nChunks = nCk;
  a.key = key;
  a.T = T;
  a.blockCnt = ctx->subCnt.as<u32>();
  a.blockOff = ctx->subOff.as<u64>();
  a.out = out.as<uint4>();
  const u32 g = grid ? grid : std::min(nBlocks, SUB_GRID);
  phase_begin(ctx, "split");
  hipLaunchKernelGGL(k_sub_count, dim3(g), dim3(SUB_NT), 0, s, a);
  if (int rc__ = dbg_sync(ctx, "k_sub_count")) return rc__;
  hipLaunchKernelGGL(k_sub_scan, dim3(1), dim3(SUB_SCAN_NT), 0, s, a.blockCnt, nBlocks, ctx->subOff.as<u64>());
  if (int rc__ = dbg_sync(ctx, "k_sub_scan")) return rc__;
  hipLaunchKernelGGL(k_sub_split, dim3(g), dim3(SUB_NT), 0, s, a);
  if (int rc__ = dbg_sync(ctx, "k_sub_split")) return rc__;
  phase_end(ctx);
  HIPCHECK(hipGetLastError());
  ctx->splitUsed = true;
  u64 total = 0;
  HIPCHECK(hipMemcpyAsync(&total, ctx->subOff.as<u64>() + nBlocks, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (total > n) {
    ctx->err = "subsample: more events kept than there are";
    return GX_ERR_DEVICE;
  }
  *nA = total;
  return GX_OK;
}

// kept sample k through the split, into its own buffer (ctx->subBufs[k])
int sub_split_kept(gx_ctx* ctx, size_t k, u64 seed, u64 T, u64* n, u64* nA) {
  if (ctx->subBufs.size() < ctx->kept.size()) ctx->subBufs.resize(ctx->kept.size());
  const CntChunk* dCk = nullptr;
  const u64* dFirst = nullptr;
  u32 nCk = 0;
  if (int rc = sub_stage(ctx, ctx->kept[k].segs, &dCk, &dFirst, &nCk, n)) return rc;
  return sub_split_pass(ctx, dCk, dFirst, nCk, *n, subsample_key(seed, (u32)k), T, 0, ctx->subBufs[k], nA);
}

void repro_drop(gx_ctx* ctx) {
  ctx->reproCalls.clear();
  ctx->reproPeaks.clear();
  ctx->splitUsed = false;
}

// one replicate's part in a call: whole (half < 0) or one of its halves
struct ReproPart { int rep, half; };
// a replicate as gx_reproducibility sees it: its treatment's and control's kept indices (-1: none), its events and half A's
struct ReproRep { int kt = -1, kc = -1; u64 n = 0, nA = 0; };

// one call: the parts as the replicates of a run on the child, each with its save mask and its control whole
int repro_call(gx_ctx* ctx, const std::vector<ReproRep>& reps, const std::vector<ReproPart>& parts, gx_repro_call& call,
               std::vector<gx_peak>& peaks) {
  gx_ctx* ch = ctx->satChild;
  peaks.clear();
  call.status = GX_OK;
  call.n_events = call.n_peaks = call.peak_bp = 0;
  for (const ReproPart& p : parts) {
    const ReproRep& R = reps[p.rep];
    call.n_events += p.half < 0 ? R.n : p.half == 0 ? R.nA : R.n - R.nA;
  }
  int rc = gx_reset(ch);
  for (size_t i = 0; !rc && i < parts.size(); i++) {
    const ReproRep& R = reps[parts[i].rep];
    const int half = parts[i].half;
    rc = gx_sample_begin(ch, 0, ctx->kept[R.kt].save.data());
    if (!rc && half < 0) rc = sat_push_whole(ch, ctx->kept[R.kt]);
    else if (!rc) {
      const u64 at = half ? R.nA : 0, m = half ? R.n - R.nA : R.nA;
      if (m) rc = gx_push_events_device(ch, ctx->subBufs[R.kt].as<gx_event>() + at, (size_t)m);
    }
    if (!rc) rc = gx_sample_end(ch, nullptr, nullptr, nullptr);
    if (rc) break;
    if (R.kc >= 0) {
      rc = gx_sample_begin(ch, 1, nullptr);
      if (!rc) rc = sat_push_whole(ch, ctx->kept[R.kc]);
      if (!rc) rc = gx_sample_end(ch, nullptr, nullptr, nullptr);
    } else
      rc = gx_sample_no_control(ch, nullptr);
    if (!rc) rc = gx_pvalues(ch);
  }
  size_t np = 0;
  uint64_t g = 0, bp = 0;
  if (!rc) rc = gx_find_peaks(ch, &np, &g, &bp);
  if (rc == GX_ERR_EXPT) {   // (the part left no analyzable fragment: a result)
    call.status = GX_ERR_EXPT;
    return GX_OK;
  }
  if (rc) {
    ctx->err = "reproducibility: " + ch->err;
    return rc;
  }
  call.n_peaks = np;
  call.peak_bp = bp;
  peaks.resize(np);
  if (np) rc = gx_get_peaks(ch, peaks.data(), np);
  return rc;
}

}  // namespace
