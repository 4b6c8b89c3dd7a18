// gx_host_call.h -- one gx_find_peaks: its plan (plan_call), and the stages that read it -- the replicates' tables, the device's
// scalars, Benjamini-Hochberg, the sweep's source.  The pieces the stages are made of are gx_host_stats.h's and gx_host_sweep.h's.
// (a part of gx_api.hip's translation unit, like its siblings)
#pragma once
namespace {

// Every decision of the call, from the context, its replicates and its switches; nothing is sized, cleared or launched here.
int plan_call(gx_ctx* ctx) {
  CallPlan& P = ctx->called = CallPlan{};
  const Knobs& K = ctx->knob;
  const bool q = ctx->par.qval_opt, one = ctx->sample == 1 && ctx->reps.size() == 1;
  const bool multi = ctx->world > 1 || ctx->forceColl;
  const PArray& r0 = ctx->reps[0];
  P.qLooseBad = ctx->qLooseBad;
  // One replicate without a control, -p, and the tile stage left the sweep's bits on the loose slots (LooseCtl): the
  // sweep walks them where they are -- no tight interval table is made unless somebody asks for it later
  const bool looseP = one && r0.loose && r0.looseSweep && !q;
  // (one replicate, no control, unit weights, -q, one rank: the tight table's kernel sums "bp at pileup V" on its way -- BH's table
  // of distinct p-values is made of those sums, not of a hash insertion per interval)
  P.packHist = q && one && r0.ctrlIsConst && !ctx->sawFrac && !multi && !K.noPackHist;
  // (round 6) ... and with -q as well, where q is a function of the pileup like p: BH's histogram is summed from the loose slots, q
  // tabulated by whole pileup (k_bh_small), the bits written from "q passes from this pileup on", the sweep as with -p -- no tight table
  const bool looseQ = P.packHist && q_loose_may(ctx) && r0.loose && r0.looseSweep && (r0.latePending || r0.lateLoose) && !ctx->hasBed;
  P.walk = looseP ? CallPlan::LOOSE_P : looseQ ? CallPlan::LOOSE_Q : CallPlan::TIGHT;
  if (P.looseSwept()) {
    // their bits are written now if lambda -- or, with -q, "q passes from this pileup on" (k_bh_small) -- came after the tile stage
    P.lateWrite = looseQ || r0.latePending;
    P.lateBefore = r0.lateLoose;
    P.specOk = looseP && !P.lateWrite && !P.lateBefore;
  }
  // the replicates: every one still in the loose slots gets its tight table, unless the sweep walks the slots; the Fisher
  // combination of several reuses the slots, so a replicate keeps what its pileup floats, if somebody asks for them, are made of
  for (size_t r = 0; r < ctx->reps.size(); r++)
    if (ctx->reps[r].loose && !P.looseSwept()) P.materialise |= (u64)1 << r;
  P.keepLoose = ctx->sample > 1;
  P.combine = ctx->sample > 1 && (int)ctx->reps.size() == ctx->sample;
  P.finalIdx = (int)ctx->reps.size() - (P.combine ? 0 : 1);
  // genome length (findPeaks 1091-1101): of the chromosomes for which the final array has p-values
  P.g = ctx->par.genome_len;
  P.genomeOpt = P.g == 0;
  if (P.genomeOpt) {
    std::vector<uint8_t> present = P.combine ? std::vector<uint8_t>(ctx->nChrom, 0) : ctx->reps[P.finalIdx].present;
    for (int r = 0; P.combine && r < ctx->sample; r++)
      for (u32 i = 0; i < ctx->nChrom; i++) present[i] |= ctx->reps[r].present[i];
    P.g = genome_len_for(ctx, present);
  }
  // the sweep's masks: whoever writes the final array fills them on the way, where there is such a one
  if (P.looseSwept()) P.masks = CallPlan::MASKS_TILE;
  else if (q) P.masks = CallPlan::MASKS_BH;
  else if (!P.combine && ((P.materialise >> P.finalIdx & 1) || (ctx->maskIdx == P.finalIdx && ctx->maskN == ctx->reps[P.finalIdx].n)))
    P.masks = CallPlan::MASKS_PACK;   // (k_pack_pval now, or the control merge's pack kernel at gx_pvalues)
  P.setMisc = q || P.masks == CallPlan::MASKS_SIG;   // (BH and k_sig_mask read them)
  if (!q) return GX_OK;
  P.bh = looseQ ? CallPlan::BH_SMALL : P.packHist && (P.materialise & 1) ? CallPlan::BH_FROM_DENSE : CallPlan::BH_FROM_HIST;
  // One sample without a control: every rank holds the same table p(V), the histogram travels as one dense all-reduce --
  // decided by what every rank knows alike
  if (multi)
    P.exchange = one && r0.ctrlIsConst && !ctx->bedGiven && (u32)std::max(1, ctx->world) <= 64 && !K.noDenseBh ? CallPlan::X_DENSE : CallPlan::X_RANGE;
  P.bhInst = bh_instance(ctx);
  P.lazyQ = looseQ || !K.noLazyQ;
  P.qtMulti = K.qtMulti != 0;
  return GX_OK;
}

// The replicates' tables: materialise, keep, combine.
int call_tables(gx_ctx* ctx, const CallPlan& P) {
  for (size_t r = 0; r < ctx->reps.size(); r++) {
    if (P.materialise >> r & 1)
      if (int rc = materialize_rep(ctx, (int)r, P.packHist)) return rc;
    if (P.keepLoose && ctx->reps[r].pilesPending)
      if (int rc = keep_loose_for_piles(ctx, (int)r)) return rc;
  }
  if (P.combine)
    if (int rc = combine_replicates(ctx)) return rc;
  ctx->finalIdx = P.finalIdx;
  return GX_OK;
}

// Genome length and interval count, for the host's mail and for the kernels that read them through pointers (BH, k_sig_mask):
// one tiny kernel instead of two copy launches, and none at all when the masks came with the p-values.
void call_scalars(gx_ctx* ctx, const CallPlan& P) {
  const u32 n = ctx->reps[P.finalIdx].n;
  ctx->genomeLenUsed = P.g;
  ctx->mail->genome = P.g;
  ctx->mail->n = n;
  if (P.setMisc) hipLaunchKernelGGL(k_set_misc, dim3(1), dim3(1), 0, ctx->stream, ctx->misc.as<u32>(), (u32)M_NIV, (u32)M_GENOME, (u64)P.g, n);
}

// Benjamini-Hochberg by the plan's route.
int call_bh(gx_ctx* ctx, const CallPlan& P) {
  PArray& fa = ctx->reps[P.finalIdx];
  if (P.bh == CallPlan::BH_NONE) return GX_OK;
  if (P.bh == CallPlan::BH_SMALL) return loose_hist(ctx, P, fa);
  phase_begin(ctx, "bh");
  BhTable T{};
  u32 Dlocal = 0, D = 0;
  if (int rc = bh_local_table(ctx, P, fa, fa.n, T, Dlocal)) return rc;
  if (int rc = bh_exchange(ctx, P, fa, fa.n, T, Dlocal, D)) return rc;
  if (D)
    if (int rc = bh_q_table(ctx, P, D)) return rc;
  if (int rc = bh_masks_and_q(ctx, P, fa, fa.n, T)) return rc;
  phase_end(ctx);
  HIPCHECK(hipGetLastError());
  return GX_OK;
}

// What the sweep walks, from the plan; the loose slots' late bits are written here.
int call_sweep_source(gx_ctx* ctx, const CallPlan& P, SweepSrc& src) {
  hipStream_t s = ctx->stream;
  u32* misc = ctx->misc.as<u32>();
  PArray& fa = ctx->reps[P.finalIdx];
  const bool looseQ = P.walk == CallPlan::LOOSE_Q;
  src = SweepSrc{};
  src.nChrom = ctx->nChrom;
  if (P.looseSwept()) {
    if (looseQ) HIPCHECK(hipMemsetAsync(ctx->swMask.p, 0, fa.looseStride * 8, s));   // (the significance words: a run before may have left its own)
    if (P.lateWrite) {
      hipLaunchKernelGGL(k_loose_late, tile_grid(ctx, 8), dim3(256), 0, s,
                         ctx->tileSlot.as<u32>(), ctx->tileIvCount.as<u32>(), ctx->tileLastEnd.as<u32>(), ctx->nTiles,
                         ctx->looseEnd.as<u32>(), ctx->looseV.as<int>(), ctx->looseCtl.as<LooseCtl>(), ctx->swMask.as<u64>(),
                         looseQ ? (const u32*)(misc + M_VQ) : (const u32*)nullptr, looseQ ? ctx->dStatus.as<u32>() : (u32*)nullptr);
      fa.latePending = false;
      fa.lateLoose = true;
      ctx->called.ran.lateWritten = true;
    }
    src.end = ctx->looseEnd.as<u32>();
    src.V = ctx->looseV.as<int>();
    src.p = ctx->pvLut.as<float>();
    if (looseQ) src.qLut = ctx->qLut.as<float>();
    src.chromOff = fa.chromLooseOff.as<u32>();
    src.mStride = fa.looseStride;
    src.nWords = (u32)(fa.looseStride - 2);
    src.haveMasks = true;
    src.hasSkip = false;
    src.specOk = P.specOk;
  } else {
    const u32 n = fa.n;
    src.end = fa.end.as<u32>();
    src.p = fa.p.as<float>();
    src.q = ctx->par.qval_opt ? fa.q.as<float>() : (const float*)nullptr;
    if (ctx->par.qval_opt && fa.qLazy) {
      src.kq = ctx->bhKQ.as<u64>();
      src.kqMask = ctx->bhLiveCap - 1;
    }
    src.chromOff = fa.chromOff.as<u32>();
    src.nWords = (n + 63) / 64;
    // the masks were filled by the pack kernels (p mode, one replicate) or by BH (q mode): whoever did left its layout behind
    src.haveMasks = P.masks != CallPlan::MASKS_SIG;
    if (src.haveMasks != (ctx->maskIdx == P.finalIdx && ctx->maskN == n)) {
      ctx->err = "peak call: the sweep's masks are not where the plan expects them";
      return GX_ERR_DEVICE;
    }
    src.mStride = src.haveMasks ? ctx->maskStride : (size_t)src.nWords + 2;
    src.hasSkip = true;
    HIPCHECK(ctx->swMask.ensure(src.mStride * 8 * 3));
    // (whoever filled the sig / skip masks zeroed all three: the chromosome-start mask is still clear)
    if (!src.haveMasks) HIPCHECK(hipMemsetAsync(ctx->swMask.p, 0, src.mStride * 8 * 3, s));
  }
  ctx->maskIdx = -1;
  return GX_OK;
}

}  // namespace
