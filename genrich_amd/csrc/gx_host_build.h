// gx_host_build.h -- a sample from its events to its run-length pileup and scalars: plan_build (every decision of a build, once), build_pileup
// (the stages the plan chose: arena, sort, tile stage, scans), finish_scalars, the retries (general chain, page tables, int16 saturation), the tile layout.
// (a part of gx_api.hip's translation unit: the kernels are templates and inline functions of the headers it includes;
// split by phase -- context / build / stats / sweep / collectives -- in round 5)
#pragma once
namespace {

uint64_t genome_len_for(const gx_ctx* ctx, const std::vector<uint8_t>& present) {
  // calcLambda 1819-1827 / findPeaks 1091-1101
  uint64_t g = 0;
  for (u32 i = 0; i < ctx->nChrom; i++)
    if (!ctx->skip[i] && present[i]) {
      g += ctx->len[i];
      for (size_t j = 0; j + 1 < ctx->bed[i].size(); j += 2) g -= ctx->bed[i][j + 1] - ctx->bed[i][j];
    }
  return g;
}

int upload_chroms(gx_ctx* ctx, bool force = true) {
  bool changed = force;
  for (u32 i = 0; i < ctx->nChrom; i++) {
    const u32 f = (ctx->skip[i] ? CH_SKIP : 0) | (ctx->save[i] ? CH_SAVE : 0) | (ctx->owned[i] ? CH_OWNED : 0);
    changed |= f != ctx->hChrom[i].flags;
    ctx->hChrom[i].flags = f;
  }
  if (!changed) return GX_OK;  // (the table on the device is this one already: no copy launch per sample)
  // (hChrom may be rewritten by the next call while this copy is in flight: pageable memory is staged by the runtime)
  HIPCHECK(hipMemcpyAsync(ctx->dChrom.p, ctx->hChrom.data(), ctx->nChrom * sizeof(DChrom), hipMemcpyHostToDevice,
                          ctx->stream));
  return GX_OK;
}

// loose slots -> tight (end, V) arrays of a pileup (only needed ahead of a control merge)
int pack_pileup(gx_ctx* ctx, Pileup& P) {
  if (P.packed) return GX_OK;
  hipStream_t s = ctx->stream;
  const u32 nTiles = ctx->nTiles;
  HIPCHECK(pooled(ctx, P.ivV, P.ivEnd.cap));
  PackIn pin{ctx->looseEnd.as<u32>(), ctx->looseV.as<int>(), ctx->tileMeta.as<TileMeta>(), P.tileIvOff.as<u32>()};
  hipLaunchKernelGGL(k_pack, tile_grid(ctx, 8), dim3(256), 0, s, pin, nTiles,
                     P.ivEnd.as<u32>(), P.ivV.as<int>());
  if (int rc__ = dbg_sync(ctx, "k_pack")) return rc__;
  P.packed = true;
  return GX_OK;
}

// gx_sample_begin's clearing of the replicate's scalars, when no k_build_init is going to do it
int flush_begin(gx_ctx* ctx) {
  if (!ctx->beginPending) return GX_OK;
  hipLaunchKernelGGL(k_begin_sample, dim3(1), dim3(64), 0, ctx->stream, ctx->dScal.as<Scalars>(), ctx->beginGenome);
  ctx->beginPending = false;
  return GX_OK;
}

// A sample about to be merged with its control stays in its loose slots (k_merge2<true> reads them there): the
// buffers leave the context -- no copy -- and the context takes others for the next build (pooled).  With -E regions
// the merge needs tight arrays after all (gx_merge.h): pack_pileup.
int stash_or_pack(gx_ctx* ctx, Pileup& P) {
  if (ctx->hasBed) return pack_pileup(ctx, P);
  if (P.inLoose) return GX_OK;
  recycle(ctx, P.looseEnd);
  recycle(ctx, P.looseV);
  recycle(ctx, P.meta);
  P.looseEnd = std::move(ctx->looseEnd);
  P.looseV = std::move(ctx->looseV);
  P.meta = std::move(ctx->tileMeta);
  P.inLoose = true;
  return GX_OK;
}

// k_sort_a's persistent grid for a piece of `chunks` chunks: what is resident together (GX_S2_GRID: tests), one chunk each at least
static u32 sort_a_grid(const gx_ctx* ctx, u32 chunks) {
  const u32 g = ctx->knob.s2Grid > 0 ? (u32)ctx->knob.s2Grid : (u32)std::max(1, ctx->resSortA);
  return std::max(1u, std::min(chunks, g));
}
// the most level-1 chunks any XCD class gets.  A chunk's class is that of the workgroup that scatters it: workgroup w of a piece's
// launch (class w % NXCD) takes the chunks w, w + grid, w + 2 grid ... -- ceil((chunks - w) / grid) of them
static u32 class_chunks(const gx_ctx* ctx) {
  u32 perClass[NXCD] = {};
  for (auto& sg : ctx->segs) {
    const u32 b = (u32)((sg.n + S2_CHUNK - 1) / S2_CHUNK), g = sort_a_grid(ctx, b);
    for (u32 w = 0; w < g && w < b; w++) perClass[w % NXCD] += (b - w + g - 1) / g;
  }
  return *std::max_element(perClass, perClass + NXCD);
}

// Packed pieces (gx_event8) -> 16-byte events, in buffers of the library: for everything that reads gx_event records -- the general
// chain's k_sort1, gx_window_net, the host's replay of the reference's int16 decisions -- and (`all` = false) for the pieces that
// k_sort_a<.., PACKED> cannot read in place: a caller's device buffer that is not 16-byte aligned or ends on an odd count.
int unpack_segs(gx_ctx* ctx, bool all) {
  size_t total = 0;
  auto wanted = [&](const gx_ctx::Seg& sg) {
    return sg.packed && sg.n && (all || (reinterpret_cast<uintptr_t>(sg.p) & 15u) || (!sg.ready && (sg.n & 1u)));
  };
  for (auto& sg : ctx->segs)
    if (wanted(sg)) total += sg.n;
  if (!total) return GX_OK;
  if (ctx->unpackUsed == ctx->unpackBufs.size()) ctx->unpackBufs.emplace_back();
  DevBuf& buf = ctx->unpackBufs[ctx->unpackUsed++];
  HIPCHECK(buf.ensure(total * sizeof(gx_event)));
  hipStream_t s = ctx->stream;
  gx_event* at = buf.as<gx_event>();
  for (auto& sg : ctx->segs) {
    if (!wanted(sg)) continue;
    if (sg.ready) HIPCHECK(hipStreamWaitEvent(s, sg.ready, 0));  // (its upload, on the side stream)
    hipLaunchKernelGGL(k_unpack_events, dim3((u32)std::min<size_t>((sg.n + 255) / 256, 8192)), dim3(256), 0, s,
                       reinterpret_cast<const uint2*>(sg.p), sg.n, reinterpret_cast<uint4*>(at));
    sg.p = at;
    sg.ready = nullptr;   // (stream-ordered from here on)
    sg.packed = false;
    at += sg.n;
  }
  HIPCHECK(hipGetLastError());
  return GX_OK;
}

// ---- a build: plan_build decides, build_pileup runs the stages it chose ----
// What a build decides, all of it, before anything is sized, cleared or launched.  Its only side effects on the context: the
// early all-reduce this rank owes from here on, and one sample of the fused stage's back-off used up.
// Several ranks: lambda needs every rank's fragLen.  Its closed form (the sum of the fragment lengths, level 1 of the sort)
// is known BEFORE the tile stage, so the ranks exchange that (`earlyColl`: one all-reduce of three words behind level 1;
// decided by what every rank knows alike) and each of them has the table p(V) and the sweep's bits from the tile stage, as
// a single rank has.  The all-reduce behind the tile stage (finish_scalars) still carries the exact parts and the ranks'
// flags; a rank whose lambda came out different there falls back to k_pack_pval as before.
int plan_build(gx_ctx* ctx, int isCtrl, bool reuseSort) {
  const Knobs& K = ctx->knob;
  BuildPlan& P = ctx->built = BuildPlan{};
  P.isCtrl = isCtrl, P.reuseSort = reuseSort;
  // (decided ahead of everything that can fail -- the size check, the allocations: a rank that leaves the build early owes
  // the others BOTH all-reduces, and poison_allreduce reads earlyOwed to know)
  P.multiRank = ctx->world > 1 || ctx->forceColl;
  const bool forceSlowFrag = K.forceSlowFrag != 0, noFused = K.noFused != 0, noLoose = K.noLoose != 0;
  P.earlyColl = P.multiRank && !isCtrl && !ctx->par.qval_opt && !ctx->bedGiven && !noLoose && !forceSlowFrag && !K.noEarlyColl;
  ctx->earlyOwed = P.earlyColl;
  // (host-pushed events sit in the library's device chunks, device-resident segments are used in place)
  size_t n = 0;
  for (auto& sg : ctx->segs) n += sg.n;
  if (2 * n >= 0xFFFFFFFFull) {
    ctx->err = "too many events in one sample for 32-bit record offsets";
    return GX_ERR_MEM;
  }
  const u32 nEv = P.nEv = (u32)n;
  const u32 nTiles = ctx->nTiles;
  // tile id + offset fit a 4-byte key (GX_FORCE_REC64=1 forces the wide-record path: used by the tests,
  // since only a genome beyond 4.29 Gbp takes it naturally)
  const bool unit32 = P.unit32 = nTiles < MAX_TILES32 && !K.forceRec64;
  const u32 nL1base = ctx->nSB - 1;  // level-1 bins = super-buckets (records without a tile are not scattered at all)
  // ---- what the tile stage will be -------------------------------------------------------------------------
  // k_sbtile (gx_sbtile.h): level 2 of the sort fused with the tile passes -- at most 2^8 tiles per super-bucket, and bins
  // that fit its LDS (a bin that does not raises ST_SB_FULL, a fractional record among unit-weight ones ST_SB_FRAC:
  // finish_scalars then has the sample built again on the general chain).  -E regions ride it since round 6 (pair mode: the
  // tiles with an edge are the second launch's, gx_sbtile.h TM_BEDX).
  // (a sample whose predecessor of the same kind did not fit is not even tried for a while: the same experiment's
  // next replicate, or the next run on the same data, has the same pile-ups)
  const bool backoff = !ctx->fusedOff && ctx->fusedBackoff[isCtrl ? 1 : 0] > 0;
  if (backoff) ctx->fusedBackoff[isCtrl ? 1 : 0]--;
  const bool pairsAllowed = !K.noPairs;
  // (fractional weights ride the pair records -- k_sort_a<true>, k_sbtile<.., true> -- once a sample of this context has
  // shown one; the start / end keys of the other fused variant cannot carry a weight)
  const bool fracOk = pairsAllowed && !K.noFracPairs;
  const bool fracLikely = ctx->sawFrac || ctx->fracHint;
  // (-E regions: unit-weight pair records only -- with a weight class as well the instances would be twelve)
  const bool fused = P.fused =
      !backoff && unit32 && (!ctx->hasBed || (pairsAllowed && !K.noBedFused && !fracLikely)) && ctx->sbShift <= SBT_MAXSHIFT && !noFused &&
      (!fracLikely || fracOk) && !ctx->fusedOff && !forceSlowFrag && (size_t)nEv <= (size_t)std::max(1u, nL1base) * 64000 &&
      (size_t)2 * nEv + nTiles + ctx->nBedEdges + 64 < ((size_t)1 << 30);  // (k_sbtile's stores use 32-bit byte offsets)
  // ... and with it level 1: one record per fragment (k_sort_a / k_sort_b) when k_sbtile will read it
  P.pairs = fused && !reuseSort && pairsAllowed;
  P.fracPairs = P.pairs && fracLikely;
  // A sample so dense that the average bin holds more keys than k_sbtile's key array (ATAC cut sites of a deep library)
  // takes bins of half the size -- level 1 of the pair mode reaches 64 x 128 of them -- so that a bin is one round of
  // the tile kernel again; the general chain (a later fall-back) keeps the context's own bin size.
  int sbS = ctx->sbShift;
  u32 nL1 = nL1base;
  // (not with fractional weights: measured at config 4, the tile passes with weights and the fragLen terms cost more per
  // key than the rounds of full-size bins -- 2.98 against 2.67 ms)
  const bool forceHalf = K.forceHalfBins != 0;  // (tests: the 128-key level 1 on a small input)
  if (P.pairs && (!P.fracPairs || forceHalf || K.fracHalfBins) && sbS > 0 &&
      (forceHalf || (size_t)2 * nEv > (size_t)std::max(1u, nL1base) * (SBT_KEYCAP - SBT_KEYCAP / 10)) &&
      ((nTiles + (1u << (sbS - 1)) - 1) >> (sbS - 1)) <= (u32)MAX_BINS_P && !K.noHalfBins) {
    sbS--;
    nL1 = (nTiles + (1u << sbS) - 1) >> sbS;
  }
  P.sbS = sbS, P.nL1 = nL1;
  // level-1 page pools (gx_sort.h): every record lands in one page of its (XCD class, bin) list
  P.jmax = ctx->ptJmax;
  // (page 0: sink; NXCD * nL1 fixed first pages; at most records / page-size further ones)
  P.poolPages[0] = P.poolPages[1] = (u32)(nEv >> PgCfg<u32>::SHIFT) + NXCD * nL1 + 4;
  P.poolPages[2] = (u32)(((size_t)2 * nEv) >> PgCfg<u64>::SHIFT) + NXCD * nL1 + 4;
  // pair mode in two passes (k_sort_a / k_sort_b): the coarse lists, and the first pass's workgroups over all pieces
  P.nCoarse = (std::max(1u, nL1) + (1u << s2_fine_shift(nL1)) - 1) >> s2_fine_shift(nL1);
  P.jmaxC = class_chunks(ctx) + 3;   // (a class's workgroups cannot fill more pages than that in one list)
  for (auto& sg : ctx->segs) P.nWG1 += (u32)((sg.n + S2_CHUNK - 1) / S2_CHUNK);
  // lambda ahead of the tile stage (closed form of fragLen; LooseCtl): one rank, a treatment sample, -p
  P.wantEarly = !isCtrl && (!P.multiRank || P.earlyColl) && !ctx->par.qval_opt && !ctx->hasBed && unit32 && !noLoose && !forceSlowFrag &&
                !ctx->sawFrac;  // (fractional weights: the closed form of fragLen is off, lambda only comes with the sample's end)
  // (round 6) ... and when lambda only comes with the sample's end -- fractional weights: no closed form of fragLen -- the sweep still
  // walks the loose slots: k_loose_late writes the bits and the fillers once the table p(V) is there (finish_scalars), instead of
  // k_pack_pval's copy of every interval into the tight table.  One rank, a treatment sample, -p, no -E regions, the fused tile stage.
  // (-q as well, where q is a function of the pileup: unit weights, no control to come -- gx_find_peaks' qLoose; a control sample
  // that follows only finds the verdict unused)
  P.wantLate = !P.wantEarly && !isCtrl && !P.multiRank && (!ctx->par.qval_opt || (q_loose_may(ctx) && !ctx->fracHint)) && !ctx->hasBed && unit32 && !noLoose &&
               !K.noLateLoose && fused && !forceSlowFrag;
  P.closeInScan = P.wantEarly && !P.multiRank;  // (k_scan_iv_close)
  P.looseCap = (size_t)2 * nEv + nTiles + ctx->nBedEdges + 16;  // slot t: records before + t (+ edges before)
  // an interval closes at every base with a non-zero difference (<= one per record), at every -E edge,
  // plus one per chromosome
  P.ivCap = (size_t)2 * nEv + ctx->nChrom + ctx->nBedEdges + 16;
  P.tChunks = (nTiles + STL_CHUNK - 1) / STL_CHUNK;
  // the tile stage is k_tile_fast (+ k_tile_heavy): the general fragLen path's terms ride in it (TileIn::fragAcc)
  // (-E regions: k_frag_walk's general path walks every interval, on either chain)
  P.fragFused = !ctx->hasBed && (!fused || P.fracPairs);
  // a sample so dense that the average bin already holds more keys than the key array (ATAC cut sites of a deep
  // library): every bin takes the rounds of k_sbtile's second launch, the first one would only find that out bin by bin
  P.dense = P.pairs && (size_t)2 * nEv > (size_t)std::max(1u, nL1) * (SBT_KEYCAP - SBT_KEYCAP / 16);
  if (P.dense) {
    // touched bases per round of the tile passes against keys per round of a bin (they share the LDS, gx_sbtile.h): what
    // costs a dense sample is the number of rounds a bin takes -- each reads the bin's records again --, so: the
    // instance with the smaller scratch when that saves the AVERAGE bin a round.  (No margin for the fuller bins: they
    // take the extra round in either instance.  Config 4, 97.8 K keys per bin against 2 x 50,048: tile stage 2.17 ms
    // with the small scratch, 2.49 with the large one, three runs each.)
    const size_t want = (size_t)2 * nEv / std::max(1u, nL1);
    auto rounds = [&](u32 tr) { return (want + sbt_keycap(tr) - 1) / sbt_keycap(tr); };
    P.denseSmall = rounds((u32)SBT_TR_DENSE) < rounds((u32)SBT_TR);
    if (K.sbtTr) P.denseSmall = K.sbtTr == SBT_TR_DENSE;   // (measurements)
  }
  return GX_OK;
}

// ---- what the stages share: views of the context as the kernels take them ---------------------------------------------------
PagedStream paged(const gx_ctx* ctx, const BuildPlan& P, int q) {
  const gx_ctx::Stream& st = ctx->str[q];
  return PagedStream{st.pool.p, st.pt.as<u32>(), st.cursor.as<u32>(), st.cursor.as<u32>() + NXCD * P.nL1, P.jmax, P.poolPages[q], NXCD * P.nL1};
}
long long* sample_acc(const gx_ctx* ctx, int isCtrl) {  // zero since gx_sample_begin(treatment)
  return isCtrl ? ctx->dScal.as<Scalars>()->ctrlAcc : ctx->dScal.as<Scalars>()->fragAcc;
}
TileIn tile_in(const gx_ctx* ctx, const BuildPlan& P) {
  TileIn tin{ctx->str[0].a.as<uint16_t>(), ctx->str[1].a.as<uint16_t>(), ctx->str[2].a.as<u64>(), ctx->tileMeta.as<TileMeta>()};
  if (P.fragFused) tin.ff = ctx->fragSum.as<FragFix>(), tin.fragAcc = sample_acc(ctx, P.isCtrl);
  return tin;
}

// Every buffer of the build, sized from the plan (the allocations only grow: a steady run finds them all large enough).
int size_buffers(gx_ctx* ctx, const BuildPlan& P, Pileup& out) {
  const u32 nTiles = ctx->nTiles, nChrom = ctx->nChrom;
  // level-2 output: 16-bit tile offsets (S, E) / whole records (F), tile-contiguous
  for (int q = 0; q < 2 && P.unit32; q++) HIPCHECK(ctx->str[q].a.ensure((size_t)P.nEv * 2 + 16));
  HIPCHECK(ctx->str[2].a.ensure((size_t)P.nEv * 16 + 16));  // worst case: every event fractional
  for (int q = 0; q < 3; q++) HIPCHECK(ctx->str[q].pool.ensure((size_t)P.poolPages[q] * PG_BYTES));
  if (P.pairs && P.nEv) {
    const u32 pagesC = P.nWG1 + 2 * NXCD * P.nCoarse + 8;
    HIPCHECK(ctx->poolC.ensure((size_t)pagesC * PG_BYTES));
    HIPCHECK(ctx->auxC.ensure((size_t)pagesC << PgCfg<u32>::SHIFT));
  }
  if (P.masks()) {
    // the sweep's masks in loose-slot index space: [significant | first of its chromosome]
    ctx->looseStride = (P.looseCap + 63) / 64 + 2;
    HIPCHECK(ctx->swMask.ensure(ctx->looseStride * 8 * 3));
    ctx->maskIdx = -1;
  }
  for (int q = 0; q < 3; q++) HIPCHECK(ctx->str[q].sbOff.ensure((MAX_BINS_P + 2) * 4));
  if (P.fused) HIPCHECK(ctx->bigBins.ensure((size_t)(MAX_BINS_P + 4) * 4));
  for (DevBuf* b : {&ctx->tileOff[0], &ctx->tileOff[1], &ctx->tileOff[2], &ctx->tileSlot, &ctx->tileCarry, &ctx->fragList, &ctx->tileIvCount,
                    &ctx->tileLastEnd, &ctx->tilePrevEnd, &ctx->wideList, &ctx->heavyList})
    HIPCHECK(b->ensure((size_t)(nTiles + 2) * 4));   // a word per tile
  HIPCHECK(ctx->chromW0.ensure((size_t)(nChrom + 1) * 4));
  // (pooled: a sample stashed for its control merge took the last ones along; chromLooseOff moves into the replicate's record)
  HIPCHECK(pooled(ctx, out.ivEnd, P.ivCap * 4));
  HIPCHECK(pooled(ctx, out.tileIvOff, (size_t)(nTiles + 2) * 4));
  HIPCHECK(pooled(ctx, out.chromIvOff, (size_t)(nChrom + 2) * 4));
  HIPCHECK(pooled(ctx, ctx->chromLooseOff, (size_t)(nChrom + 2) * 4));
  HIPCHECK(pooled(ctx, ctx->looseEnd, P.looseCap * 4));
  HIPCHECK(pooled(ctx, ctx->looseV, P.looseCap * 4));
  HIPCHECK(pooled(ctx, ctx->tileMeta, (size_t)(nTiles + 1) * sizeof(TileMeta)));
  return GX_OK;
}

// everything that must start at zero lives in one arena: one launch per sample clears it (k_build_init: with the sweep's masks and the
// replicate's scalars).  (The order matters to clear_arena: a repeated tile stage clears from tileCnt[0] to the end.)
int carve_arena(gx_ctx* ctx, const BuildPlan& P) {
  const u32 nTiles = ctx->nTiles;
  auto lay = [&](char* base) {   // hands out 256-aligned views in the order they are asked for; without a base it only adds up
    size_t at = 0;
    auto take = [&](DevBuf& v, size_t bytes) {
      if (base) v.view(base + at, (bytes + 255) & ~(size_t)255);
      at += (bytes + 255) & ~(size_t)255;
    };
    const size_t tileBytes = (size_t)(nTiles + 1) * 4, lists = (size_t)NXCD * P.nL1, listsC = (size_t)NXCD * P.nCoarse;
    take(ctx->fragSum, sizeof(FragFix));
    take(ctx->nWide, 256);
    take(ctx->looseCtl, sizeof(LooseCtl));
    take(ctx->endAtLen, (size_t)(ctx->nChrom + 1) * 4);
    take(ctx->binNet, (size_t)(MAX_BINS_P + 2) * 4);  // pair mode: the singles' weight per level-1 bin
    take(ctx->curC, listsC * 4 + 64);                 // pair mode's coarse lists: cursors and page tables
    take(ctx->ptC, listsC * P.jmaxC * 4);
    for (int q = 0; q < 3; q++) {
      take(ctx->str[q].cursor, lists * 4 + 64);       // cursors + (last word) pages handed out
      take(ctx->str[q].pt, lists * P.jmax * 4);
    }
    for (int q = 0; q < 3; q++) take(ctx->tileCnt[q], tileBytes);
    take(ctx->tileWsum, tileBytes);
    take(ctx->tileDeep, tileBytes);
    take(ctx->lb, (size_t)3 * (P.tChunks + 2) * 8);   // k_scan_tiles' three look-back arrays
    take(ctx->lbIv, (size_t)(2 * P.tChunks + 4) * 8); // k_scan_iv's two
    return at;
  };
  ctx->arenaBytes = lay(nullptr);
  HIPCHECK(ctx->zeroArena.ensure(ctx->arenaBytes));
  lay(ctx->zeroArena.as<char>());
  return GX_OK;
}

int clear_arena(gx_ctx* ctx, const BuildPlan& P) {
  hipStream_t s = ctx->stream;
  if (!P.reuseSort) {
    const size_t nA = ctx->arenaBytes / 16, nB = P.masks() ? ctx->looseStride * 8 * 2 / 16 : 0;
    static_assert(sizeof(Scalars) / 8 <= 256, "one workgroup clears the scalars");
    hipLaunchKernelGGL(k_build_init, dim3((u32)std::min<size_t>((nA + nB + 1023) / 1024, 4096)), dim3(256), 0, s, ctx->dScal.as<Scalars>(),
                       ctx->beginPending ? 1 : 0, ctx->beginGenome, ctx->zeroArena.as<uint4>(), nA, P.masks() ? ctx->swMask.as<uint4>() : (uint4*)nullptr, nB);
    ctx->beginPending = false;
    return GX_OK;
  }
  // reuseSort: level 1 of the sort -- the pages, the cursors, the closed form of fragLen -- is still there.  What goes is what the
  // tile stage and the scans of the first attempt left: the per-tile tables and look-back arrays (the arena's tail), the
  // loose-sweep block, the correction words of fragLen and the wide-tile count
  if (int rc__ = flush_begin(ctx)) return rc__;
  if (P.masks()) HIPCHECK(hipMemsetAsync(ctx->swMask.p, 0, ctx->looseStride * 8 * 2, s));
  char* tail = ctx->tileCnt[0].as<char>();
  HIPCHECK(hipMemsetAsync(tail, 0, (size_t)(ctx->zeroArena.as<char>() + ctx->arenaBytes - tail), s));
  HIPCHECK(hipMemsetAsync(ctx->looseCtl.p, 0, ctx->looseCtl.cap, s));
  HIPCHECK(hipMemsetAsync(&ctx->fragSum.as<FragFix>()->nList, 0, 12, s));   // nList, corr (the partial sums and the slow flag stay)
  HIPCHECK(hipMemsetAsync(nw_word(ctx, NW_WIDE), 0, 4, s));  // (NW_HOT, the int16 flag of level 1, stays)
  HIPCHECK(hipMemsetAsync(nw_word(ctx, NW_HEAVY), 0, 4, s));
  return GX_OK;
}

// level 1 of the sort: every piece's events -> paged lists per (XCD class, bin); the closed form of fragLen on the way
int sort_level1(gx_ctx* ctx, const BuildPlan& P) {
  hipStream_t s = ctx->stream;
  FragFix* ff = ctx->fragSum.as<FragFix>();
  // fragLen: closed form (sum of fragment lengths) unless something sets the slow flag
  // (-E regions: the fused tile stage takes the excluded bases' pileup off the closed form, FragFix::bedExcl; k_tile<BED> does not)
  if ((ctx->hasBed && !P.fused) || !P.unit32 || ctx->knob.forceSlowFrag) HIPCHECK(hipMemsetAsync(&ff->slow, 1, 4, s));
  if (P.reuseSort) return dbg_sync(ctx, "k_sort1");
  const PagedStream PG0 = paged(ctx, P, 0), PG1 = paged(ctx, P, 1), PG2 = paged(ctx, P, 2);
  const Sort1Out so1{ff->fragSum, &ff->slow, ctx->endAtLen.as<u32>(), nw_word(ctx, NW_HOT)};
  // two passes for pair records: coarse bins, then the fine ones (gx_sort.h)
  const u32 nListsC = NXCD * P.nCoarse;
  const PagedStream PC{ctx->poolC.p, ctx->ptC.as<u32>(), ctx->curC.as<u32>(), ctx->curC.as<u32>() + nListsC, P.jmaxC, P.nWG1 + 2 * nListsC + 8, nListsC};
  static constexpr decltype(&k_sort_a<false, false>) SORT_A[2][2] = {{k_sort_a<false, false>, k_sort_a<false, true>},   // [FRAC][PACKED]
                                                                     {k_sort_a<true, false>, k_sort_a<true, true>}};
  for (auto& seg : ctx->segs) {
    if (!seg.n) continue;
    // (a piece that is still on its way from the host: the main stream waits for that copy only, so the
    // scatter of the pieces that have arrived overlaps the upload of the rest)
    if (seg.ready) HIPCHECK(hipStreamWaitEvent(s, seg.ready, 0));
    const u32 blocks = (u32)((seg.n + S1_CHUNK - 1) / S1_CHUNK);
    if (P.pairs) {
      // (a piece of 8-byte events by the instance that reads those in place)
      hipLaunchKernelGGL(SORT_A[P.fracPairs][seg.packed], dim3(sort_a_grid(ctx, blocks)), dim3(S2_NT), 0, s, seg.p, (u32)seg.n, ctx->dChrom.as<DChrom>(), ctx->nChrom, P.sbS,
                         P.nL1, P.nCoarse, PC, ctx->auxC.as<uint8_t>(), PG2, ctx->binNet.as<int>(), so1, ctx->dStatus.as<u32>());
      ctx->packedUsed |= seg.packed;
    } else
      hipLaunchKernelGGL(P.unit32 ? k_sort1<true> : k_sort1<false>, dim3(blocks), dim3(S1_NT), 0, s, seg.p, (u32)seg.n,
                         ctx->dChrom.as<DChrom>(), ctx->nChrom, P.sbS, P.nL1, PG0, PG1, PG2, so1, ctx->dStatus.as<u32>());
  }
  if (P.pairs && P.nEv) {
    // the coarse lists (all pieces' events) -> the fine bins' lists.  A class's lists hold at most its chunks' + one partly filled page
    // each; the resident workgroups (a multiple of NXCD: the same number for every class) share them
    const u32 want = ctx->knob.s2Grid > 0 ? (u32)ctx->knob.s2Grid : (u32)std::max(1, ctx->resSortB);
    const u32 gridB = std::min((u32)NXCD * (P.jmaxC - 3 + P.nCoarse), (want + NXCD - 1) / NXCD * NXCD);
    hipLaunchKernelGGL(k_sort_b, dim3(gridB), dim3(S2_NT), 0, s, PC, (const uint8_t*)ctx->auxC.as<uint8_t>(),
                       P.nCoarse, P.nL1, PG0, ctx->dStatus.as<u32>());
  }
  return dbg_sync(ctx, "k_sort1");
}

// several ranks: this rank's closed form of fragLen, whether it is valid here (unit weights so far, no -E regions, 4-byte keys), [2] unused
long long* early_words(const gx_ctx* ctx, const BuildPlan& P) { return P.earlyColl ? ctx->dColl.as<long long>() + 4 : nullptr; }
int early_allreduce(gx_ctx* ctx, const BuildPlan& P) {
  if (!P.earlyColl) return GX_OK;
  hipLaunchKernelGGL(k_early_words, dim3(1), dim3(64), 0, ctx->stream, ctx->fragSum.as<FragFix>(), P.wantEarly ? 0 : 1, early_words(ctx, P));
  if (int rc__ = allreduce_words(ctx, early_words(ctx, P), 3)) return rc__;
  ctx->earlyOwed = false;
  return GX_OK;
}

// the bins' offsets from level 1's cursors; with an early lambda also the table p(V) for it, and from which pileup on an interval is significant
int scan_bins(gx_ctx* ctx, const BuildPlan& P) {
  gx_ctx::Stream* S = ctx->str;
  auto capOf = [&](int shift) -> u32 { return P.jmax >= (1u << (31 - shift)) ? 0x7FFFFFFFu : P.jmax << shift; };  // (list_cap)
  BinScan bs{{S[0].cursor.as<u32>(), S[1].cursor.as<u32>(), S[2].cursor.as<u32>()},
             {capOf(PgCfg<u32>::SHIFT), capOf(PgCfg<u32>::SHIFT), capOf(PgCfg<u64>::SHIFT)},
             {S[0].sbOff.as<u32>(), S[1].sbOff.as<u32>(), S[2].sbOff.as<u32>()},
             ctx->endAtLen.as<u32>(), ctx->chromW0.as<int>(), ctx->nChrom, ctx->fragSum.as<FragFix>(), ctx->dScal.as<Scalars>(), ctx->looseCtl.as<LooseCtl>(),
             P.wantEarly ? 1 : 0, P.pairs ? 1 : 0, ctx->binNet.as<int>(), nw_word(ctx, NW_NEED_PAGES), early_words(ctx, P)};
  static_assert(PV_LUT % 1024 == 0, "k_bins_lut: four of k_pval_lut's workgroups per block");
  if (P.wantEarly)
    hipLaunchKernelGGL(k_bins_lut, dim3(4 + PV_LUT / 1024), dim3(1024), 0, ctx->stream, bs, P.nL1, ctx->pvLut.as<float>(),
                       ctx->dRisk.as<RiskBuf>(), ctx->dDeep.as<DeepTab>(), ctx->par.thr, ctx->dStatus.as<u32>());
  else
    hipLaunchKernelGGL(k_scan_bins, dim3(4), dim3(1024), 0, ctx->stream, bs, P.nL1);
  return GX_OK;
}

// the general chain's level 2: one workgroup per super-bucket and stream, then the tiles' offsets and descriptors
int general_level2(gx_ctx* ctx, const BuildPlan& P) {
  hipStream_t s = ctx->stream;
  const u32 nTiles = ctx->nTiles;
  gx_ctx::Stream* S = ctx->str;
  const size_t lds2 = std::max(b2_lds_bytes<u32>(1u << P.sbS), b2_lds_bytes<u64>(1u << P.sbS));
  if (ctx->b2LdsSet != lds2) {
    HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_bucket2p), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    ctx->b2LdsSet = lds2;
  }
  // (the F stream: multimapped reads, or everything beyond 4.29 Gbp; a run without them finds every bin empty)
  Bucket2Jobs BJ{{{paged(ctx, P, 0), S[0].a.p, S[0].sbOff.as<u32>(), ctx->tileCnt[0].as<u32>()},
                  {paged(ctx, P, 1), S[1].a.p, S[1].sbOff.as<u32>(), ctx->tileCnt[1].as<u32>()},
                  {paged(ctx, P, 2), S[2].a.p, S[2].sbOff.as<u32>(), ctx->tileCnt[2].as<u32>()}}};
  hipLaunchKernelGGL(k_bucket2p, dim3(std::max(1u, P.nL1), 3), dim3(B2_NT), lds2, s, BJ, P.nL1, P.sbS, nTiles, ctx->tileWsum.as<int>());
  if (int rc__ = dbg_sync(ctx, "k_bucket2p")) return rc__;
  TileTabs tt{};
  for (int q = 0; q < 3; q++) tt.cnt[q] = ctx->tileCnt[q].as<u32>(), tt.off[q] = ctx->tileOff[q].as<u32>();
  tt.wsumF = ctx->tileWsum.as<int>(), tt.prefW = ctx->tileCarry.as<int>();
  u64* lb = ctx->lb.as<u64>();
  hipLaunchKernelGGL(k_scan_tiles, dim3(std::min<u32>(P.tChunks, (u32)ctx->resSweep)), dim3(STL_NT), 0, s, tt, nTiles, lb, lb + P.tChunks + 2,
                     lb + 2 * (P.tChunks + 2), ctx->dStatus.as<u32>());
  if (int rc__ = dbg_sync(ctx, "k_scan_tiles")) return rc__;
  hipLaunchKernelGGL(k_tile_meta, dim3((nTiles + 255) / 256), dim3(256), 0, s, ctx->tileOff[0].as<u32>(), ctx->tileOff[1].as<u32>(),
                     ctx->tileOff[2].as<u32>(), ctx->tileCarry.as<int>(), ctx->dTileChrom.as<u32>(), ctx->dChrom.as<DChrom>(),
                     ctx->hasBed ? ctx->dBedTileOff.as<u32>() : (const u32*)nullptr, nTiles, ctx->tileMeta.as<TileMeta>(), ctx->wideList.as<u32>(),
                     nw_word(ctx, NW_WIDE), ctx->tileSlot.as<u32>(), ctx->hasBed ? (u32*)nullptr : ctx->heavyList.as<u32>());
  return GX_OK;
}

// The instances of k_sbtile, each named here and nowhere else: what raises their dynamic-LDS limit walks this table, a launch looks its own up in it.
using SbtKernel = void (*)(SbtIn, SbtOut, u32*);
struct SbtInstance { bool pairs, big, frac; int trc; bool bed; SbtKernel fn; };
#define GX_SBT(PAIRS, BIG, FRAC, TRC, BED) {PAIRS, BIG, FRAC, TRC, BED, k_sbtile<PAIRS, BIG, FRAC, TRC, BED>}
const SbtInstance SBT_INSTANCES[] = {
    GX_SBT(false, false, false, SBT_TR, false),                                                     // start / end keys (GX_NO_PAIRS)
    GX_SBT(true, false, false, SBT_TR, false),      GX_SBT(true, true, false, SBT_TR, false),       // pair records: first and second launch
    GX_SBT(true, false, true, SBT_TR, false),       GX_SBT(true, true, true, SBT_TR, false),        // ... with a weight class
    GX_SBT(true, false, false, SBT_TR, true),       GX_SBT(true, true, false, SBT_TR, true),        // ... with -E regions
    GX_SBT(true, true, false, SBT_TR_DENSE, false), GX_SBT(true, true, true, SBT_TR_DENSE, false), GX_SBT(true, true, false, SBT_TR_DENSE, true),  // dense
};
#undef GX_SBT

int launch_sbtile(gx_ctx* ctx, bool pairs, bool big, bool frac, int trc, bool bed, dim3 grid, const SbtIn& si, const SbtOut& so) {
  if (!ctx->sbtLdsSet) {
    for (const SbtInstance& k : SBT_INSTANCES)
      HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SBT_LDS_BYTES));
    ctx->sbtLdsSet = true;
  }
  for (const SbtInstance& k : SBT_INSTANCES)
    if (k.pairs == pairs && k.big == big && k.frac == frac && k.trc == trc && k.bed == bed) {
      hipLaunchKernelGGL(k.fn, grid, dim3(SBT_NT), SBT_LDS_BYTES, ctx->stream, si, so, ctx->dStatus.as<u32>());
      return GX_OK;
    }
  ctx->err = "no k_sbtile instance <" + std::to_string(pairs) + ", " + std::to_string(big) + ", " + std::to_string(frac) + ", " + std::to_string(trc) +
             ", " + std::to_string(bed) + ">";
  return GX_ERR_DEVICE;
}

// the tile stage: loose (end, V) slots and interval counts per tile
int tile_stage(gx_ctx* ctx, const BuildPlan& P) {
  hipStream_t s = ctx->stream;
  const u32 nTiles = ctx->nTiles;
  FragFix* ff = ctx->fragSum.as<FragFix>();
  long long* acc = sample_acc(ctx, P.isCtrl);
  const TileIn tin = tile_in(ctx, P);
  // (the sweep's bits written late: LooseCtl::enabled stays 0 -- no bits, no fillers; a pileup beyond the table still says so)
  const TileOut to{ctx->looseEnd.as<u32>(), ctx->looseV.as<int>(), ctx->tileIvCount.as<u32>(), ctx->tileLastEnd.as<u32>(), ctx->tileDeep.as<u32>(),
                   P.masks() ? ctx->swMask.as<u64>() : (u64*)nullptr, P.masks() ? ctx->looseCtl.as<LooseCtl>() : (LooseCtl*)nullptr};
  const BedIn bin{ctx->dBedTileOff.as<u32>(), ctx->dBedEdge.as<u32>(), ctx->dTileSave0.as<uint8_t>()};
  if (P.fused) {
    // level 2 of the sort and the tile passes in one kernel, one workgroup per super-bucket (gx_sbtile.h)
    gx_ctx::Stream* S = ctx->str;
    const bool fragIn = P.fragFused && P.fracPairs;
    const SbtIn si{paged(ctx, P, 0), paged(ctx, P, 1), paged(ctx, P, 2), S[0].sbOff.as<u32>(), S[1].sbOff.as<u32>(), S[2].sbOff.as<u32>(),
                   ctx->dTileChrom.as<u32>(), ctx->dChrom.as<DChrom>(), ctx->chromW0.as<int>(), P.nL1, nTiles, P.sbS,
                   fragIn ? (const FragFix*)ff : (const FragFix*)nullptr, fragIn ? acc : (long long*)nullptr,
                   ctx->hasBed ? bin : BedIn{nullptr, nullptr, nullptr}, ctx->hasBed ? ff->fragSum : (u64*)nullptr};
    SbtOut so{to, ctx->tileMeta.as<TileMeta>(), ctx->tileSlot.as<u32>(), nw_word(ctx, NW_HOT), nw_word(ctx, NW_NBIG),
              ctx->bigBins.as<u32>(), ctx->heavyList.as<u32>(), nw_word(ctx, NW_HEAVY), nw_word(ctx, NW_SBT_TICKET)};
    const dim3 gAll(std::max(1u, P.nL1)), gBig(std::max(1u, std::min(P.nL1, (u32)ctx->numCU)));
    // the first launch is persistent: a workgroup per CU (160 KiB of LDS: there is room for one), each drawing bins from the
    // ticket word -- in the arena k_build_init clears, so zero for every sample and every rebuild (GX_SBT_GRID: tests, A/B)
    const dim3 gPers(std::max(1u, std::min(gBig.x, ctx->knob.sbtGrid > 0 ? (u32)ctx->knob.sbtGrid : gBig.x)));
    const bool frac = P.fracPairs, bed = P.pairs && !frac && ctx->hasBed;
    int rc;
    if (P.dense) {  // every bin by the second launch's rounds
      so.bigList = nullptr;
      rc = launch_sbtile(ctx, true, true, frac, P.denseSmall ? SBT_TR_DENSE : SBT_TR, bed, gAll, si, so);
    } else {
      rc = launch_sbtile(ctx, P.pairs, false, frac, SBT_TR, bed, gPers, si, so);
      // the bins it left on its list (reads piled up: more keys than the key array holds, a tile with thousands of keys):
      // usually none -- an idle launch
      // (-E regions: the bins with an edge tile are the second launch's as well -- every second bin of hg38 with ~800 regions, so
      // a workgroup per bin of the grid, dealt by the dispatcher; the ones beyond the list leave at once)
      if (!rc && P.pairs) rc = launch_sbtile(ctx, true, true, frac, SBT_TR, bed, bed ? gAll : gBig, si, so);
    }
    if (rc) return rc;
  } else {
    // narrow tiles with 16-bit LDS counters (twice the tiles in flight), then the wide ones from their list
    // (whose length stays on the device: an empty list costs one idle launch)
    const u32 *wl = ctx->wideList.as<u32>(), *nw = nw_word(ctx, NW_WIDE);
    if (ctx->hasBed) {
      const dim3 gHalf(std::min<u32>(nTiles, (u32)ctx->resTileHalf)), gWide(std::min<u32>(nTiles, (u32)ctx->resTile));
      hipLaunchKernelGGL((k_tile<true, true>), gHalf, dim3(TL_NT), TL_LDS_HALF * 4, s, tin, nTiles, wl, nw, bin, to, ctx->dStatus.as<u32>());
      hipLaunchKernelGGL((k_tile<true, false>), gWide, dim3(TL_NT), TL_LDS * 4, s, tin, nTiles, wl, nw, bin, to, ctx->dStatus.as<u32>());
    } else {
      // the common case: one wavefront per tile, work laid out by touched base, unit-weight and fractional records alike (gx_tile_fast.h)
      hipLaunchKernelGGL(k_tile_fast, dim3(std::min<u32>(nTiles, (u32)ctx->resTileFast)), dim3(64), 0, s, tin, nTiles, nw, to, ctx->dStatus.as<u32>());
      // the tiles with thousands of records (pile-ups): a workgroup each, a counter per base (usually none: an idle launch)
      hipLaunchKernelGGL(k_tile_heavy, dim3(64), dim3(TH_NT), 0, s, tin, ctx->heavyList.as<u32>(), nw_word(ctx, NW_HEAVY), to, ctx->dStatus.as<u32>());
    }
  }
  return dbg_sync(ctx, "k_tile");
}

// NW_HOT, the "a base can reach the int16 limits" flag (also set by level 1 of the sort), on the general chain
// (a bin that fits k_sbtile holds fewer than 32,767 records of a stream: no base of it can reach the limits)
// (a tile that can hold such a base has >= 32,766 records: it is on the list of the heavy tiles -- walking the list of
// the WIDE tiles instead cost config 4, where every tile holds fractional records and is "wide", 2.1 ms of header reads)
int hot_check(gx_ctx* ctx, const BuildPlan& P) {
  if (!P.fused) {
    const bool haveHeavy = !ctx->hasBed;
    hipLaunchKernelGGL(k_hot_check, dim3(std::min<u32>(ctx->nTiles, 256u)), dim3(256), 0, ctx->stream, tile_in(ctx, P),
                       haveHeavy ? ctx->heavyList.as<u32>() : ctx->wideList.as<u32>(), nw_word(ctx, haveHeavy ? NW_HEAVY : NW_WIDE),
                       nw_word(ctx, NW_HOT));
  }
  return dbg_sync(ctx, "k_hot_check");
}

// the general fragLen path's walk over the listed tiles, then (single thread: chromosome offsets of the chromosomes without tiles, closed
// form -> accumulator pair, this rank's words of the all-reduce) the sample's closing, from the arguments the build left in closeSel
void launch_frag_close(gx_ctx* ctx, const Pileup& out) {
  const u32 nTiles = ctx->nTiles;
  hipLaunchKernelGGL(k_frag_walk, dim3(std::max(1u, std::min((nTiles + 3) / 4, 4096u))), dim3(256), 0, ctx->stream,
                     ctx->looseEnd.as<u32>(), ctx->looseV.as<int>(), ctx->tileMeta.as<TileMeta>(), out.tileIvOff.as<u32>(),
                     ctx->tilePrevEnd.as<u32>(), nTiles, ctx->fragSum.as<FragFix>(), ctx->fragList.as<u32>(), ctx->closeSel.acc,
                     ctx->built.fragFused ? ctx->heavyList.as<u32>() : (const u32*)nullptr, nw_word(ctx, NW_HEAVY));
  hipLaunchKernelGGL(k_frag_select, dim3(1), dim3(1), 0, ctx->stream, ctx->closeSel);
}

// ---- what the sweep's run pass needs, shared by run_sweep and by the pass launched ahead of time (spec_runs) -----------------
// persistent workgroups of a look-back kernel of the sweep (GX_SWEEP_GRID: tests)
u32 sweep_grid(const gx_ctx* ctx, int resident) {
  const u32 g = (u32)std::max(1, resident);
  return ctx->knob.sweepGrid > 0 ? std::min(g, (u32)ctx->knob.sweepGrid) : g;
}
// the runs the sweep's arrays are sized for (never more runs than intervals)
u32 sweep_run_cap(const gx_ctx* ctx, u32 nWords) {
  const u64 capMin = ctx->knob.runCapMin > 0 ? (u64)ctx->knob.runCapMin : (u64)1 << 16;  // (tests: a tiny first guess)
  // (first guess: one run per 256 intervals -- several times what a default threshold leaves on a genome --
  // so that a single call does not pay for a second pass)
  const u64 guess = ctx->knob.runCapMin > 0 ? capMin : std::max<u64>(capMin, (u64)nWords / 4);
  return (u32)std::min<u64>(std::max<u64>(ctx->runCap, std::max<u64>(guess, 1)), (u64)nWords * 64);
}
// the run arrays for `cap` runs and the run pass's look-back granules (generation-tagged: never cleared between calls)
int sweep_run_arrays(gx_ctx* ctx, u32 cap, u32 wChunks) {
  HIPCHECK(ctx->swStart.ensure((size_t)cap * 4 + 16));
  HIPCHECK(ctx->swEnd.ensure((size_t)cap * 4 + 16));
  const size_t need = (size_t)2 * (wChunks + 8) * 8;
  if (ctx->lbSweep.cap < need) {
    HIPCHECK(ctx->lbSweep.ensure(need));
    HIPCHECK(hipMemsetAsync(ctx->lbSweep.p, 0, ctx->lbSweep.cap, ctx->stream));
  }
  return GX_OK;
}
int sweep_next_gen(gx_ctx* ctx, u32* gen) {
  if (++ctx->sweepGen >= (1u << 24)) {  // (the generation field wraps: start over with clean arrays)
    ctx->sweepGen = 1;
    if (ctx->lbSweep.cap) HIPCHECK(hipMemsetAsync(ctx->lbSweep.p, 0, ctx->lbSweep.cap, ctx->stream));
    if (ctx->lbSweep2.cap) HIPCHECK(hipMemsetAsync(ctx->lbSweep2.p, 0, ctx->lbSweep2.cap, ctx->stream));
  }
  *gen = ctx->sweepGen;
  return GX_OK;
}
RunsOut runs_out(gx_ctx* ctx, u32 cap) {
  u32* misc = ctx->misc.as<u32>();
  HostMail* dm = static_cast<HostMail*>(ctx->mailBuf.dp);
  return RunsOut{ctx->swStart.as<u32>(), ctx->swEnd.as<u32>(), cap, misc + M_SWCOUNT, &dm->R, misc + M_TICKET3,
                 reinterpret_cast<u64*>(misc + M_PEAKBP)};
}
// the chromosomes' first loose slots, from what the tile stage left (ChromStarts)
ChromStarts chrom_starts(const gx_ctx* ctx) { return ChromStarts{ctx->dChrom.as<DChrom>(), ctx->tileSlot.as<u32>(), ctx->nChrom}; }

// May the sweep's run pass ride in the scan's launch?  A treatment sample whose tile stage wrote the sweep's bits (lambda known
// early), -p, one rank, built for the first time.  Whether the sweep will be the one this pass is for -- one replicate, no control,
// the loose slots accepted -- only gx_find_peaks knows: run_sweep takes the pass or drops it.
bool spec_runs_wanted(const gx_ctx* ctx, const BuildPlan& P) {
  return P.closeInScan && P.wantEarly && !P.wantLate && !P.multiRank && !P.isCtrl && !P.fracPairs && !ctx->par.qval_opt && ctx->buildAttempt == 0 &&
         ctx->sample == 0 && !ctx->knob.noSweepOverlap && !ctx->knob.noLoose && ctx->looseStride > 2;
}

// tile-local interval counts -> offsets (the pass over the tiles for fragLen -- deep-tile list, long first intervals --
// rides in the scan), then the sample's closing: in the scan's own launch when lambda was known before the tile stage
int scan_and_close(gx_ctx* ctx, const BuildPlan& P, Pileup& out) {
  const u32 nTiles = ctx->nTiles;
  FragFix* ff = ctx->fragSum.as<FragFix>();
  LooseCtl* ctl = ctx->looseCtl.as<LooseCtl>();
  long long* acc = sample_acc(ctx, P.isCtrl);
  u32* nIv = ctx->misc.as<u32>() + M_NIV;
  const IvScanOut so{out.tileIvOff.as<u32>(), ctx->tilePrevEnd.as<u32>(), out.chromIvOff.as<u32>(), nIv, ctx->tileSlot.as<u32>(),
                     ctx->chromLooseOff.as<u32>(), ctx->looseEnd.as<u32>(), ctx->looseV.as<int>(), ctl, ctx->tileDeep.as<u32>(), ff,
                     ctx->fragList.as<u32>(), P.fragFused ? acc : (long long*)nullptr, ctx->endAtLen.as<u32>()};
  ctx->closeSel = FragSelect{ff, acc, P.multiRank ? ctx->dColl.as<long long>() : (long long*)nullptr, nw_word(ctx, NW_HOT),
                             ctx->dStatus.as<u32>(), ctx->dChrom.as<DChrom>(), ctx->nChrom, out.chromIvOff.as<u32>(), nIv,
                             ctx->dScal.as<Scalars>(), P.isCtrl, ctx->chromLooseOff.as<u32>(), ctx->tileSlot.as<u32>(), nTiles, ctl,
                             P.masks() ? ctx->swMask.as<u64>() + ctx->looseStride : (u64*)nullptr};
  ctx->closeSeq = P.closeInScan ? ++ctx->mailSeq : 0;   // (the mail k_scan_iv_close sends)
  // k_scan_iv, or -- with a CloseArgs -- k_scan_iv_close: the same launch but for the last argument
  auto scan = [&](auto kernel, auto... close) {
    hipLaunchKernelGGL(kernel, dim3(std::min<u32>(P.tChunks, (u32)ctx->resSweep)), dim3(STL_NT), 0, ctx->stream, ctx->tileIvCount.as<u32>(),
                       ctx->tileLastEnd.as<u32>(), ctx->dTileChrom.as<u32>(), ctx->dChrom.as<DChrom>(), nTiles, ctx->lbIv.as<u64>(),
                       ctx->lbIv.as<u64>() + P.tChunks + 1, so, ctx->dStatus.as<u32>(), close...);
  };
  ctx->specRuns.valid = false;
  if (!P.closeInScan) scan(k_scan_iv);
  if (int rc__ = dbg_sync(ctx, "k_scan_iv")) return rc__;
  if (!P.closeInScan)
    launch_frag_close(ctx, out);
  else {
    // k_frag_select's work and the mail ride in the scan's launch (its last workgroup closes the sample); if a deep tile,
    // the general fragLen path or a changed lambda stands in the way, finish_scalars runs the separate kernels after all
    ctx->mail->nMerged = ctx->mail->closeState = 0;
    HostMail* dm = static_cast<HostMail*>(ctx->mailBuf.dp);
    const CloseArgs ca{ctx->closeSel, nIv, (const u32*)&ctl->ok, ctx->dRisk.as<RiskBuf>(), mail_out(ctx), &dm->closeState,
                       ctx->closeSeq, nw_word(ctx, NW_CLOSE_TICKET)};
    if (spec_runs_wanted(ctx, P)) {
      // ... and so does the sweep's run pass, in workgroups of its own behind the scan's: it needs the tile stage's bits only
      const u32 nWords = (u32)(ctx->looseStride - 2), wChunks = (nWords + SW_CHUNK - 1) / SW_CHUNK;
      const u32 cap = sweep_run_cap(ctx, nWords);
      if (int rc__ = sweep_run_arrays(ctx, cap, wChunks)) return rc__;
      u32 gen = 0;
      if (int rc__ = sweep_next_gen(ctx, &gen)) return rc__;
      // both halves resident together: each half's own bound, and if the two do not fit, half of the kernel's residency each
      const u32 res = (u32)std::max(2, ctx->resScanRuns);
      u32 gScan = std::min<u32>(P.tChunks, sweep_grid(ctx, ctx->resSweep)), gRun = std::min<u32>(wChunks, sweep_grid(ctx, ctx->resSweep));
      if (gScan + gRun > res) {
        gScan = std::min<u32>(gScan, res / 2);
        gRun = std::min<u32>(gRun, res - gScan);
      }
      u64* lbS = ctx->lbSweep.as<u64>();
      const RunHalf rh{SweepMasks{ctx->swMask.as<u64>(), nullptr, ctx->swMask.as<u64>() + ctx->looseStride, nWords}, chrom_starts(ctx),
                       lbS, lbS + wChunks + 8, gen, runs_out(ctx, cap), gScan};
      hipLaunchKernelGGL(k_scan_iv_close_runs, dim3(gScan + gRun), dim3(STL_NT), 0, ctx->stream, ctx->tileIvCount.as<u32>(),
                         ctx->tileLastEnd.as<u32>(), ctx->dTileChrom.as<u32>(), ctx->dChrom.as<DChrom>(), nTiles, ctx->lbIv.as<u64>(),
                         ctx->lbIv.as<u64>() + P.tChunks + 1, so, ctx->dStatus.as<u32>(), ca, rh);
      ctx->specRuns = gx_ctx::SpecRuns{true, gen, cap, nWords, ctx->looseStride};
    } else
      scan(k_scan_iv_close, ca);
    if (int rc__ = dbg_sync(ctx, "k_close")) return rc__;
  }
  if (int rc__ = dbg_sync(ctx, "k_frag")) return rc__;
  out.packed = out.inLoose = false;
  if (P.isCtrl)  // a control is always merged against the treatment
    if (int rc__ = stash_or_pack(ctx, out)) return rc__;
  return GX_OK;
}

// events -> tile-bucketed endpoint records -> run-length pileup (loose slots + offsets) and fragLen.  reuseSort: the sample was built a moment
// ago and only its tile stage has to be done again on the general chain (k_sbtile sent it back): level 1 of the sort is still there.
int build_pileup(gx_ctx* ctx, Pileup& out, int isCtrl, bool reuseSort = false) {
  if (int rc = plan_build(ctx, isCtrl, reuseSort)) return rc;
  const BuildPlan& P = ctx->built;
  int rc;
  ctx->packedUsed = false;
  // (8-byte events: k_sort_a reads them in place; everything else -- and a piece it cannot read in place -- gets 16-byte copies)
  if (!reuseSort && (rc = unpack_segs(ctx, !P.pairs))) return rc;
  if ((rc = size_buffers(ctx, P, out))) return rc;
  if ((rc = carve_arena(ctx, P))) return rc;
  if ((rc = clear_arena(ctx, P))) return rc;
  phase_begin(ctx, isCtrl ? "c.sort1" : "t.sort1");
  if ((rc = sort_level1(ctx, P))) return rc;
  phase_end(ctx);
  if (ctx->knob.fault == 1 && !reuseSort) HIPCHECK(hipMemsetAsync(ctx->endAtLen.p, 0x01, 4, ctx->stream));  // (tests: ST_END_PILE must catch it)
  if ((rc = early_allreduce(ctx, P))) return rc;
  phase_begin(ctx, isCtrl ? "c.bucket" : "t.bucket");
  if ((rc = scan_bins(ctx, P))) return rc;
  if (!P.fused && (rc = general_level2(ctx, P))) return rc;
  phase_end(ctx);
  phase_begin(ctx, isCtrl ? "c.tile" : "t.tile");  // the tile kernels alone: the dominant ones (bench.py's roofline)
  if ((rc = tile_stage(ctx, P))) return rc;
  phase_end(ctx);
  if ((rc = hot_check(ctx, P))) return rc;
  phase_begin(ctx, isCtrl ? "c.pack" : "t.pack");
  if ((rc = scan_and_close(ctx, P, out))) return rc;
  phase_end(ctx);
  HIPCHECK(hipGetLastError());
  ctx->nIvTarget = &out.nIv;  // filled from the mail block once finish_scalars has synchronised
  return GX_OK;
}

constexpr int RETRY_GENERAL = 3;    // (internal) k_sbtile could not take the sample: build it again on the general chain
constexpr int RETRY_SATURATED = 1;  // (internal) finish_scalars: filter the events and build the sample again
constexpr int RETRY_PT = 2;         // (internal) a level-1 page list overflowed: build again with a longer page table
// (the page tables -- NXCD x bins x jmax x 4 bytes, three streams -- at the cap and hg38's 2,946 bins: 18.5 GB, which a
// 288 GB device holds; 2^20, round 2's cap, would have asked for 50 GB per stream.  A list beyond 2^16 pages holds
// more than 5 x 10^8 keys of ONE super-bucket: such a sample fails with "could not be rebuilt")
constexpr u32 PT_JMAX_CAP = 1u << 16;

// fragLen / ctrlFrag partial sums -> (all ranks) -> lambda, factor
int finish_scalars(gx_ctx* ctx, int isCtrl) {
  hipStream_t s = ctx->stream;
  Scalars* ds = ctx->dScal.as<Scalars>();
  const bool multi = ctx->world > 1 || ctx->forceColl;
  long long* dcoll = multi ? ctx->dColl.as<long long>() : nullptr;
  if (multi) {
    // The third word sums the ranks' "build this sample again" flags, so that every rank learns from the one
    // synchronisation below whether the sums are final.
    if (int rc__ = allreduce_words(ctx, dcoll, 3)) return rc__;
    ctx->earlyPending = false;
    // (one rank: k_frag_select has done it).  With lambda known to every rank before the tile stage (the build's early
    // all-reduce), this is also where a rank learns whether its sweep bits were written with the
    // lambda that turned out final.
    hipLaunchKernelGGL(k_finish_frag, dim3(1), dim3(1), 0, s, ds, isCtrl, ctx->dStatus.as<u32>(), (const long long*)dcoll,
                       !isCtrl && ctx->built.earlyColl ? ctx->looseCtl.as<LooseCtl>() : (LooseCtl*)nullptr);
    if (int rc__ = dbg_sync(ctx, "k_finish_frag")) return rc__;
  }
  bool closed = false;
  if (ctx->closeSeq) {
    // k_scan_iv_close has sent the mail (scan_and_close); only if something stood in its way do the separate kernels run
    if (int rc__ = mail_wait(ctx, ctx->closeSeq)) return rc__;
    ctx->closeSeq = 0;
    closed = ctx->mail->closeState == 1;
    if (!closed) {
      ctx->specRuns.valid = false;   // (a deep tile, the general fragLen path, another lambda: the sweep's bits may not be final)
      launch_frag_close(ctx, ctx->expt);  // (closed in the scan: a treatment sample)
      if (int rc__ = dbg_sync(ctx, "k_frag (after k_close)")) return rc__;
    }
  }
  if (!closed) {
  // lambda (and with a control the factor) is final: build the p-value tables now, so that the values the
  // host has to re-evaluate (risky ones) travel with the synchronisation that returns the scalars
  if (!isCtrl) {
    PackIn pin{ctx->looseEnd.as<u32>(), ctx->looseV.as<int>(), ctx->tileMeta.as<TileMeta>(), ctx->expt.tileIvOff.as<u32>()};
    // (when the tile stage had lambda already -- LooseCtl -- and it has not changed, only the deep tiles' part runs)
    hipLaunchKernelGGL(k_pval_lut, dim3(PV_LUT / 256 + DEEP_BLOCKS), dim3(256), 0, s, ds, ctx->pvLut.as<float>(),
                       ctx->dRisk.as<RiskBuf>(), ctx->dDeep.as<DeepTab>(), pin, ctx->fragSum.as<FragFix>(),
                       ctx->fragList.as<u32>(), ctx->looseCtl.as<LooseCtl>(), ctx->built.wantLate ? 2 : 0, ctx->par.thr);
    // (lambda came with the sample's end: may the sweep walk the loose slots?  The pass that writes its bits runs when gx_find_peaks
    // finds the replicate to be the run's only one -- gx_stats.h k_loose_late)
    if (ctx->built.wantLate) hipLaunchKernelGGL(k_loose_verdict, dim3(1), dim3(256), 0, s, ctx->looseCtl.as<LooseCtl>());
  } else {
    hipLaunchKernelGGL(k_pair_tabs, dim3(PAIR_LUT / 256), dim3(256), 0, s, ds, ctx->pairLogE.as<double>(),
                       ctx->pairCtab.as<CtrlEntry>());
    hipLaunchKernelGGL(k_pair_tab2d, dim3(PT_N * PT_N / 256), dim3(256), 0, s, ds, ctx->pairLogE.as<double>(),
                       ctx->pairCtab.as<CtrlEntry>(), ctx->pairP2d.as<float>(), ctx->dRisk.as<RiskBuf>());
    ctx->pairTabsReady = true;
  }
  if (int rc__ = dbg_sync(ctx, "p-value tables")) return rc__;
  ctx->mail->nMerged = 0;
  if (int rc__ = mail_sync(ctx, ds, nw_word(ctx, NW_HOT), ctx->misc.as<u32>() + M_NIV, dcoll,
                           isCtrl ? (const u32*)nullptr : &ctx->looseCtl.as<LooseCtl>()->ok))
    return rc__;
  }
  ctx->hScal = ctx->mail->scal;
  if (ctx->hScal.fracSeen) ctx->sawFrac = true;  // (learned, not hinted: the next sample does without the early lambda)
  ctx->riskNearThr = false;
  const int rcRisk = risk_apply(ctx, RiskTargets{});
  if (!isCtrl) ctx->looseOk = ctx->mail->nMerged != 0 && !ctx->riskNearThr;
  // (with several ranks: if any of them has to rebuild its sample, all go round again with it)
  const long long again = multi ? ctx->mail->coll[2]
                                : (long long)(ctx->mail->hot ? 1 : 0) + ((ctx->mail->status & ST_PT_FULL) ? 65536 : 0) +
                                      ((ctx->mail->status & (ST_SB_FULL | ST_SB_FRAC)) ? (1ll << 32) : 0);
  if (again >> 48) {
    ctx->err = "another rank could not build its sample";
    return GX_ERR_DEVICE;
  }
  if (again >> 32) {
    // k_sbtile could not take some rank's sample (a bin beyond its LDS, or fractional weights): once more, on the
    // general chain
    // (fractional weights in a unit-weight build: its singles may also have overfilled a bin -- that says nothing about
    // the next sample, which writes pair records with a weight class)
    if (ctx->knob.debugRetry) fprintf(stderr, "[gx] sample sent back to the general chain: status %u (fused %d pairs %d frac %d)\n",
                                          ctx->mail->status, (int)ctx->built.fused, (int)ctx->built.pairs, (int)ctx->built.fracPairs);
    if (ctx->mail->status & ST_SB_FRAC) ctx->sawFrac = true;
    else if (ctx->mail->status & ST_SB_FULL) ctx->fusedBackoff[isCtrl ? 1 : 0] = 8;
    ctx->fusedOff = true;
    ctx->fellBack = true;
    static_cast<RiskBuf*>(ctx->riskHost.p)->count = 0;
    HIPCHECK(hipMemsetAsync(ctx->dRisk.p, 0, 4, s));
    return RETRY_GENERAL;
  }
  if ((again & 0xFFFFFFFFll) >= 65536 && ctx->ptJmax < PT_JMAX_CAP) return RETRY_PT;
  int rc = status_to_rc(ctx, ctx->mail->status);
  if ((again & 0xFFFF) && !ctx->satDone) return RETRY_SATURATED;
  if (ctx->nIvTarget) *ctx->nIvTarget = ctx->mail->nIv;
  ctx->nIvTarget = nullptr;
  return rc ? rc : rcRisk;
}

// what a build that is repeated left behind: its status bits and its part of fragLen / ctrlFrag
int wipe_build(gx_ctx* ctx, int isCtrl) {
  HIPCHECK(hipMemsetAsync(ctx->dStatus.p, 0, 64, ctx->stream));
  HIPCHECK(hipMemsetAsync(sample_acc(ctx, isCtrl), 0, 16, ctx->stream));
  return GX_OK;
}

// The sample holds a base that can reach the reference's int16 limits: bring the events to the host,
// drop the ones saveInterval would drop (gx_saturate.h) and stage what is left for a second build.
int drop_saturated(gx_ctx* ctx, int isCtrl) {
  hipStream_t s = ctx->stream;
  if (int rc__ = unpack_segs(ctx, true)) return rc__;   // (the replay reads gx_event records)
  size_t total = 0;
  for (auto& sg : ctx->segs) total += sg.n;
  std::vector<gx_event> all(total);
  size_t at = 0;
  HIPCHECK(hipStreamSynchronize(ctx->side));  // (the uploads have long arrived: the sample was built once)
  for (auto& sg : ctx->segs) {  // in push order: the replay depends on it
    if (sg.n) HIPCHECK(hipMemcpyAsync(all.data() + at, sg.p, sg.n * sizeof(gx_event), hipMemcpyDeviceToHost, s));
    at += sg.n;
  }
  HIPCHECK(hipStreamSynchronize(s));
  // only the chromosomes this context works on (the others' events are ignored by level 1 of the sort too)
  std::vector<uint32_t> len(ctx->nChrom);
  for (u32 i = 0; i < ctx->nChrom; i++) len[i] = ctx->hChrom[i].tileBase == NULL_TILE ? 0u : ctx->len[i];
  std::vector<uint8_t> keep(total);
  const long long dropped = gxsat::filter(all.data(), total, (int)ctx->nChrom, len.data(), keep.data());
  ctx->satDropped = dropped > 0 ? dropped : 0;
  size_t kept = 0;
  if (dropped > 0) {
    for (size_t i = 0; i < total; i++)
      if (keep[i]) all[kept++] = all[i];
  } else
    kept = total;
  // (also when nothing was dropped: the second build must not see the caller's segments twice)
  HIPCHECK(ctx->satBuf.ensure(std::max<size_t>(kept, 1) * sizeof(gx_event)));
  if (kept) HIPCHECK(hipMemcpyAsync(ctx->satBuf.p, all.data(), kept * sizeof(gx_event), hipMemcpyHostToDevice, s));
  HIPCHECK(hipStreamSynchronize(s));  // `all` goes out of scope
  ctx->segs.clear();
  if (kept) ctx->segs.push_back({ctx->satBuf.as<gx_event>(), kept, nullptr});
  ctx->satDone = true;
  return wipe_build(ctx, isCtrl);
}

int close_sample(gx_ctx* ctx, Pileup& P, int isCtrl) {
  ctx->fusedOff = false;
  if (!isCtrl) ctx->looseOk = false;
  bool reuseSort = false;
  for (int attempt = 0; attempt < 12; attempt++) {
    ctx->buildAttempt = attempt;
    int rc = build_pileup(ctx, P, isCtrl, reuseSort);
    reuseSort = false;
    if (rc) {
      // With several ranks the others are about to wait for this one in the fragLen all-reduce: take part in it with a
      // "this rank has failed" word, so that every rank returns an error instead of one returning and the rest hanging.
      const std::string why = ctx->err;
      poison_allreduce(ctx);
      ctx->err = why;
      return rc;
    }
    rc = finish_scalars(ctx, isCtrl);
    if (rc == RETRY_GENERAL) {
      // k_sbtile could not take the sample (finish_scalars has switched it off for this one): the general chain,
      // on the pages level 1 of the sort has already filled
      if (int w = wipe_build(ctx, isCtrl)) return w;
      // (pair records are of no use to the general chain: level 1 runs again as start / end keys)
      reuseSort = !ctx->built.pairs;
      if (reuseSort) {
        // (k_sort1 does not run again: the status bits IT raised -- bad counts, positions, chromosomes -- must survive)
        // (and only those: what the abandoned tile stage raised -- e.g. "negative pileup" from carries that count the
        // dropped ends of fractional records it never saw -- means nothing)
        ctx->mail->statusKeep = ctx->mail->status & (ST_BAD_CHROM | ST_BAD_POS | ST_BAD_COUNT | ST_PT_FULL | ST_LOOKBACK);
        HIPCHECK(hipMemcpyAsync(ctx->dStatus.p, &ctx->mail->statusKeep, 4, hipMemcpyHostToDevice, ctx->stream));
      }
    } else if (rc == RETRY_PT) {
      // a (XCD class, super-bucket) list needed more pages than its table row holds -- reads piled up in one
      // spot: what the first build left behind goes, the table grows, the sample is built again
      // ... to what the longest list asked for (k_scan_bins: the cursors count every reservation), with a quarter to
      // spare -- not by a blind factor: the table is NXCD x bins x jmax words per stream, cleared for every sample
      u32 need = 0;
      HIPCHECK(hipMemcpy(&need, nw_word(ctx, NW_NEED_PAGES), 4, hipMemcpyDeviceToHost));
      u32 want = std::max(ctx->ptJmax * 2, need + need / 4 + 2);
      ctx->ptJmax = std::min(want, PT_JMAX_CAP);
      ctx->ptGrew = true;
      if (int w = wipe_build(ctx, isCtrl)) return w;
    } else if (rc == RETRY_SATURATED) {
      if ((rc = drop_saturated(ctx, isCtrl))) return rc;  // (sets satDone: finish_scalars asks for this once)
    } else
      return rc;
  }
  ctx->err = "sample could not be rebuilt";
  return GX_ERR_DEVICE;
}

// tile space, super-buckets, -E edge lists and the chromosome table for the chromosomes this
// context works on: not skipped (-e), not empty, and owned by this rank (gx_set_owned)
int layout_tiles(gx_ctx* ctx) {
  const int n = (int)ctx->nChrom;
  const std::vector<uint32_t>& len = ctx->len;
  ctx->hChrom.assign(n, DChrom{});
  std::vector<u32> tileChrom;
  u32 t = 0;
  for (int i = 0; i < n; i++) {
    DChrom& c = ctx->hChrom[i];
    c.len = len[i];
    if (ctx->skip[i] || !ctx->owned[i] || len[i] == 0) {
      c.tileBase = NULL_TILE;
      c.nTiles = 0;
      continue;
    }
    c.tileBase = t;
    c.nTiles = (u32)(((uint64_t)len[i] + TILE - 1) >> TB);
    for (u32 k = 0; k < c.nTiles; k++) tileChrom.push_back((u32)i);
    t += c.nTiles;
  }
  if (t == 0) {
    // a rank that owns nothing still needs a (dormant) tile space: the first analyzable chromosome's
    for (int i = 0; i < n && t == 0; i++)
      if (!ctx->skip[i] && len[i] != 0) {
        DChrom& c = ctx->hChrom[i];
        c.tileBase = 0;
        c.nTiles = (u32)(((uint64_t)len[i] + TILE - 1) >> TB);
        tileChrom.assign(c.nTiles, (u32)i);
        t = c.nTiles;
      }
  }
  ctx->nTiles = t;
  if (t == 0) {
    ctx->err = "No analyzable genome (length=0)";
    return GX_ERR_GEN;
  }
  int lg = 0;
  while ((1u << lg) < t) lg++;
  // tiles per super-bucket: the level-1 scatter wants few bins (long runs per bin and chunk); level 2 wants
  // a super-bucket's keys to fit its one-pass LDS sort (45 K keys: ~2^9 tiles at hg38 / 50 M fragments) and
  // enough super-buckets for every CU; GX_SBSHIFT overrides for experiments
  // (k_sbtile, the fused level 2 + tile kernel, takes super-buckets of up to 2^8 tiles: hg38 = 2,946 bins)
  ctx->sbShift = std::min(SBT_MAXSHIFT, std::max(0, (lg - 1) / 2));
  if (ctx->knob.sbShift >= 0) ctx->sbShift = std::max(0, std::min(11, ctx->knob.sbShift));
  while (((t + (1u << ctx->sbShift) - 1) >> ctx->sbShift) + 1 > (u32)MAX_BINS) ctx->sbShift++;
  if ((1u << ctx->sbShift) > (u32)MAX_BINS) {
    ctx->err = "genome too large for the two-level tile sort";
    return GX_ERR_MEM;
  }
  ctx->nSB = ((t + (1u << ctx->sbShift) - 1) >> ctx->sbShift) + 1;  // + the null bucket
  // -E edges per tile (Genrich.c:2185-2195: a region starting at 0 only flips the initial state)
  {
    std::vector<u32> bedOff(t + 1, 0), edges;
    std::vector<uint8_t> save0(t, 1);
    ctx->hasBed = false;
    for (int i = 0; i < n; i++) {
      const DChrom& c = ctx->hChrom[i];
      if (c.tileBase == NULL_TILE) continue;
      const std::vector<uint32_t>& b = ctx->bed[i];
      if (!b.empty()) ctx->hasBed = true;
      bool state = b.empty() || b[0] != 0;
      size_t k = (!b.empty() && b[0] == 0) ? 1 : 0;
      for (u32 tl = 0; tl < c.nTiles; tl++) {
        const uint64_t lo = (uint64_t)tl << TB, hi = lo + TILE;
        save0[c.tileBase + tl] = state;
        bedOff[c.tileBase + tl] = (u32)edges.size();
        while (k < b.size() && b[k] < hi && b[k] < c.len) {
          edges.push_back((u32)(b[k] - lo));
          state = !state;
          k++;
        }
      }
    }
    bedOff[t] = (u32)edges.size();
    ctx->nBedEdges = edges.size();
    HIPCHECK(ctx->dBedTileOff.ensure((size_t)(t + 1) * 4));
    HIPCHECK(ctx->dBedEdge.ensure(edges.size() * 4 + 16));
    HIPCHECK(ctx->dTileSave0.ensure((size_t)t + 16));
    HIPCHECK(hipMemcpy(ctx->dBedTileOff.p, bedOff.data(), (size_t)(t + 1) * 4, hipMemcpyHostToDevice));
    if (!edges.empty()) HIPCHECK(hipMemcpy(ctx->dBedEdge.p, edges.data(), edges.size() * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->dTileSave0.p, save0.data(), (size_t)t, hipMemcpyHostToDevice));
  }
  HIPCHECK(ctx->dChrom.ensure((size_t)n * sizeof(DChrom)));
  HIPCHECK(ctx->dTileChrom.ensure((size_t)t * 4));
  HIPCHECK(hipMemcpyAsync(ctx->dTileChrom.p, tileChrom.data(), (size_t)t * 4, hipMemcpyHostToDevice, ctx->stream));
  return upload_chroms(ctx);
}

}  // namespace
