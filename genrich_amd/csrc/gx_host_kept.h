// gx_host_kept.h -- the host frame of the per-sample passes.  The kept samples: which events each keeps (keep_sample), the views
// a pass sees them through and what it stages for the device (kept_stage / kept_send), a caller's host events as one more view
// (kept_upload), the events per view (kept_sizes), the driver of the passes that take the views one at a time (kept_each_view).
// And the list a kernel fills and counts, run once more when it ran full (counted_list, counted_list_read).
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
// each view's events and the chunks kept_stage cuts them into
struct ViewSize { u64 n, nCk; };
std::vector<ViewSize> kept_sizes(const std::vector<KeptView>& views) {
  std::vector<ViewSize> z(views.size(), ViewSize{0, 0});
  for (size_t v = 0; v < views.size(); v++)
    for (const gx_ctx::Seg& sg : *views[v].segs) {
      z[v].n += sg.n;
      z[v].nCk += (sg.n + CNT_CHUNK - 1) / CNT_CHUNK;
    }
  return z;
}
int kept_stage(gx_ctx* ctx, const std::vector<KeptView>& views, size_t front, bool wantChroms, bool wantFirst, KeptIn& in) {
  const u32 nChrom = ctx->nChrom;
  const std::vector<ViewSize> z = kept_sizes(views);
  in.chunk0.assign(views.size() + 1, 0);
  for (size_t v = 0; v < views.size(); v++) in.chunk0[v + 1] = in.chunk0[v] + (size_t)z[v].nCk;
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

// a caller's n host events (packed: gx_event8 records) as the pieces of one view: one upload into ctx->hookEv, which the *_events
// hooks share like keptStage / keptIn -- each drains the stream before it returns.  (A hook's refusals that depend on n alone
// come before this call: nothing is allocated for a call that is refused.)
int kept_upload(gx_ctx* ctx, const void* ev, size_t n, bool packed, std::vector<gx_ctx::Seg>& segs) {
  segs.clear();
  if (!n) return GX_OK;
  const size_t bytes = n * (packed ? sizeof(gx_event8) : sizeof(gx_event));
  POOLED(ctx, ctx->hookEv, bytes);
  HIPCHECK(hipMemcpyAsync(ctx->hookEv.p, ev, bytes, hipMemcpyHostToDevice, ctx->stream));
  segs.push_back({ctx->hookEv.as<gx_event>(), n, nullptr, packed});
  return GX_OK;
}

// the kept samples' rep / ctrl on their results
template <class R>
void kept_stamp(const gx_ctx* ctx, std::vector<R>& res) {
  for (size_t k = 0; k < res.size(); k++) {
    res[k].rep = ctx->kept[k].rep;
    res[k].ctrl = ctx->kept[k].ctrl;
  }
}

// The passes that take the views one at a time (complexity, interval stats; the kept samples or a caller's events alike): the
// views staged with their chromosome tables behind a front of `front` bytes that fill(host, device) writes, one copy, the
// stream drained, then pass(dCk, nCk, dCh, v) for view after view.  (The caller's refusals come first.)
template <class Fill, class Pass>
int kept_each_view(gx_ctx* ctx, const std::vector<KeptView>& views, size_t front, Fill fill, Pass pass) {
  KeptIn in;
  if (int rc = kept_stage(ctx, views, front, true, false, in)) return rc;
  fill(in.front, in.dFront);
  if (int rc = kept_send(ctx, in)) return rc;
  HIPCHECK(hipStreamSynchronize(ctx->stream));   // (a view without events launches nothing: the staging area is free again)
  for (size_t v = 0; v < views.size(); v++)
    if (int rc = pass(in.dCk + in.chunk0[v], (u32)(in.chunk0[v + 1] - in.chunk0[v]), in.dCh + v * ctx->nChrom, v)) return rc;
  return GX_OK;
}
template <class Pass>
int kept_each_view(gx_ctx* ctx, const std::vector<KeptView>& views, Pass pass) {
  return kept_each_view(ctx, views, 0, [](char*, const char*) {}, pass);
}

// A list that a kernel appends to and counts past its end: `out` holds `words` control words and counters, of which
// out[iStatus] & fullBit says that the list ran full and out[iCount] how many entries there were to append.
struct CountedList {
  const char *figure, *noun;         // the messages: "<figure>: a <noun> of 2^32 entries or more", "<figure>: the <noun> ran full twice"
  DevBuf* list;
  size_t esz;                        // bytes per entry
  DevBuf* out;
  size_t words;
  u32 iStatus, iCount;
  u64 fullBit, badBit;               // badBit: a status bit that ends the pass, before the full list is looked at (0: none) ...
  const char* badText;               // ... with its sentence
  u64 cap;                           // in: the first pass's capacity; out: the last pass's
  u32 reruns = 0;                    // out: 0 or 1
};
// One pass with a list of `cap` entries: the words cleared, launch(cap), the words read into h[words].  When the list ran
// full, once more with a list of the counted size, which holds every entry.
template <class Launch>
int counted_list(gx_ctx* ctx, CountedList& L, std::vector<unsigned long long>& h, Launch launch) {
  hipStream_t s = ctx->stream;
  for (L.reruns = 0;; L.reruns++) {
    if (L.cap >> 32) return refuse(ctx, std::string(L.figure) + ": a " + L.noun + " of 2^32 entries or more");
    POOLED(ctx, *L.list, (size_t)std::max<u64>(L.cap, 1) * L.esz);
    HIPCHECK(hipMemsetAsync(L.out->p, 0, L.words * 8, s));
    if (int rc = launch((u32)L.cap)) return rc;
    HIPCHECK(hipMemcpyAsync(h.data(), L.out->p, L.words * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (h[L.iStatus] & L.badBit) {
      ctx->err = L.badText;
      return GX_ERR_DEVICE;
    }
    if (!(h[L.iStatus] & L.fullBit)) return GX_OK;
    if (L.reruns || h[L.iCount] <= L.cap) {
      ctx->err = std::string(L.figure) + ": the " + L.noun + " ran full twice";
      return GX_ERR_DEVICE;
    }
    L.cap = h[L.iCount];
  }
}
// the list's n entries to the host, ascending in key(entry) (they come in the order of the races: nobody sees it)
template <class E, class Key>
int counted_list_read(gx_ctx* ctx, const DevBuf& list, u64 n, Key key, std::vector<E>& e) {
  e.resize((size_t)n);
  if (!n) return GX_OK;
  HIPCHECK(hipMemcpyAsync(e.data(), list.p, (size_t)n * sizeof(E), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  std::sort(e.begin(), e.end(), [&](const E& a, const E& b) { return key(a) < key(b); });
  return GX_OK;
}

}  // namespace
