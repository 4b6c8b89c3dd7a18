// gx_api.hip -- C ABI (include/genrich_amd.h) over the HIP kernels.  Host code here only
// sizes buffers, launches kernels on one stream and moves scalars; every per-base /
// per-interval computation of the hot path runs on the device.  There is no CPU fallback:
// a missing device or a failed launch is reported as GX_ERR_DEVICE.
#include "gx_host_ctx.h"
#include "gx_host_coll.h"
#include "gx_host_build.h"
#include "gx_host_sweep.h"
#include "gx_host_stats.h"
#include "gx_host_call.h"
#include "gx_sparse.h"
#include "gx_peak_merge.h"
#include "gx_host_kept.h"
#include "gx_host_count.h"
#include "gx_host_regions.h"
#include "gx_host_coverage.h"
#include "gx_host_profile.h"
#include "gx_host_binstat.h"
#include "gx_host_gram.h"
#include "gx_host_fingerprint.h"
#include "gx_host_rank.h"
#include "gx_host_complexity.h"
#include "gx_host_ivstat.h"
#include "gx_host_xcor.h"
#include "gx_host_gcbias.h"
#include "gx_host_motifs.h"
#include "gx_host_kmers.h"
#include "gx_host_subsample.h"
#include "gx_host_depth.h"
#include "gx_host_peaksig.h"
#include "gx_host_summits.h"

namespace {

// The entry checks the passes between samples repeat, with the function's name in their sentences.
int guard_closed(gx_ctx* ctx, const char* fn) {
  if (ctx->phase == 1 || ctx->phase == 3) return refuse(ctx, std::string(fn) + ": a sample is open");
  return GX_OK;
}
// ... of the passes over the kept samples: counting on; with needSample, no sample open and at least one closed
int guard_kept(gx_ctx* ctx, const char* fn, bool needSample) {
  if (!ctx->countOn) return refuse(ctx, std::string(fn) + " needs the samples' intervals kept (gx_set_count_in_peaks)");
  if (!needSample) return GX_OK;
  if (int rc = guard_closed(ctx, fn)) return rc;
  if (ctx->kept.empty()) return refuse(ctx, std::string(fn) + ": no closed sample");
  return GX_OK;
}

// A sample's result summed over contexts (each works on chromosomes of its own): every context has its results
// (ready(c)), as many as context 0 and compatible with them (same(c, c0, r, r0)); add(sum, r) adds one.
template <class R, class Ready, class Same, class Add>
int group_sum(gx_ctx* const* ctxs, int n_ctx, int sample, std::vector<R> gx_ctx::*results, Ready ready, Same same, Add add, R& sum) {
  if (!ctxs || n_ctx < 1) return GX_ERR_ORDER;
  for (int g = 0; g < n_ctx; g++) {
    const gx_ctx* c = ctxs[g];
    if (!c || !ready(c) || sample < 0 || (size_t)sample >= (c->*results).size() || (c->*results).size() != (ctxs[0]->*results).size() ||
        !same(c, ctxs[0], (c->*results)[sample], (ctxs[0]->*results)[sample]))
      return GX_ERR_ORDER;
    if (g == 0) sum = (c->*results)[sample];
    else add(sum, (c->*results)[sample]);
  }
  return GX_OK;
}
template <class R>
bool same_sample(const R& r, const R& r0) { return r.rep == r0.rep && r.ctrl == r0.ctrl; }
constexpr auto any_goes = [](const auto&...) { return true; };

int depth_sum(gx_ctx* const* ctxs, int n_ctx, int sample, gx_ctx::DepthResult& sum) {
  return group_sum(ctxs, n_ctx, sample, &gx_ctx::depth, [](const gx_ctx* c) { return c->phase != 1 && c->phase != 3; }, any_goes, depth_add, sum);
}
int cpx_sum(gx_ctx* const* ctxs, int n_ctx, int sample, gx_ctx::CpxResult& sum) {
  return group_sum(ctxs, n_ctx, sample, &gx_ctx::cpx, [](const gx_ctx* c) { return c->cpxReady; }, any_goes, cpx_add, sum);
}
int ivs_sum(gx_ctx* const* ctxs, int n_ctx, int sample, gx_ctx::IvsResult& sum) {
  return group_sum(ctxs, n_ctx, sample, &gx_ctx::ivs, [](const gx_ctx* c) { return c->ivsReady; },
                   [](const gx_ctx*, const gx_ctx*, const auto& r, const auto& r0) { return r.cn.size() == r0.cn.size() && same_sample(r, r0); }, ivs_add, sum);
}
int xc_sum(gx_ctx* const* ctxs, int n_ctx, int sample, gx_ctx::XcResult& sum) {
  return group_sum(ctxs, n_ctx, sample, &gx_ctx::xc, any_goes,
                   [](const gx_ctx* c, const gx_ctx* c0, const auto& r, const auto& r0) { return c->xcLo == c0->xcLo && c->xcHi == c0->xcHi && same_sample(r, r0); },
                   xc_add, sum);
}
int gc_sum(gx_ctx* const* ctxs, int n_ctx, int sample, gx_ctx::GcResult& sum) {
  return group_sum(ctxs, n_ctx, sample, &gx_ctx::gcRes, [](const gx_ctx* c) { return c->gcReady; },
                   [](const gx_ctx*, const gx_ctx*, const auto& r, const auto& r0) { return r.W == r0.W && same_sample(r, r0); }, gc_add, sum);
}
// The writers over contexts live in this file, not in gx_emit.cpp: they read contexts, and that file links on its own, against the
// entries its stand-alone test programs define.  Those that run their pass themselves:
// pass(ctx, &n) on every context, which all report as many samples (*nS)
template <class Pass>
int pass_on_all(gx_ctx* const* ctxs, int n_ctx, Pass pass, int* nS) {
  for (int g = 0; g < n_ctx; g++) {
    int n = 0;
    if (int rc = pass(ctxs[g], &n)) return rc;
    if (g && n != *nS) return GX_ERR_ORDER;
    *nS = n;
  }
  return GX_OK;
}

}  // namespace

// ================================ C ABI ==================================================

extern "C" {

const char* gx_strerror(int status) {
  switch (status) {
    case GX_OK: return "";
    case GX_ERR_MEM: return "Cannot allocate memory";
    case GX_ERR_GEN: return "No analyzable genome (length=0)";
    case GX_ERR_EXPT: return "Experimental sample has no analyzable fragments";
    case GX_ERR_PILE: return "Invalid pileup value (< 0)";
    case GX_ERR_POS: return ": read aligned beyond reference end";
    case GX_ERR_ALNS: return "Disallowed number of alignments";
    case GX_ERR_ARR: return "Failure creating experimental pileup";
    case GX_ERR_PVAL: return "Failure collecting p-values";
    case GX_ERR_DF: return "Invalid df in pchisq()";
    case GX_ERR_ORDER: return "API called out of order";
    case GX_ERR_DEVICE: return "HIP device failure";
    default: return "Unknown error";
  }
}

int gx_create(gx_ctx** out, const gx_params* par) {
  if (!out || !par) return GX_ERR_ORDER;
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= par->device) {
    fprintf(stderr, "genrich_amd: no HIP device %d (found %d) -- there is no CPU fallback\n", par->device, nd);
    return GX_ERR_DEVICE;
  }
  gx_ctx* ctx = new gx_ctx();
  ctx->par = *par;
  ctx->device = par->device;
  for (const KnobDef& d : KNOBS)
    if (const char* e = getenv(d.name)) set_knob(ctx->knob, d.name, e);
  if (ctx->knob.bhCapLog) ctx->bhCapLog = (u32)std::max(4, std::min(28, ctx->knob.bhCapLog));  // (tests: a tiny first table)
  if (ctx->knob.ptJmax) ctx->ptJmax = (u32)std::max(1, std::min(1 << 16, ctx->knob.ptJmax));   // (tests: short page-table rows)
  *out = ctx;
  HIPCHECK(hipSetDevice(ctx->device));
  HIPCHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  HIPCHECK(ctx->mailBuf.ensure(sizeof(HostMail)));
  ctx->mail = static_cast<HostMail*>(ctx->mailBuf.p);
  memset(ctx->mail, 0, sizeof(HostMail));
  HIPCHECK(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
  HIPCHECK(hipEventCreateWithFlags(&ctx->sideEv, hipEventDisableTiming));
  HIPCHECK(ctx->misc.ensure(M_WORDS * 4));
  HIPCHECK(ctx->dScal.ensure(sizeof(Scalars)));
  HIPCHECK(ctx->dStatus.ensure(64));
  // p-value tables and the list of risky values: fixed sizes, built while a sample is closed
  HIPCHECK(ctx->pvLut.ensure((size_t)(PV_LUT + PV_WHOLE) * 4));  // p(V), and p of the whole pileups once more (compact)
  HIPCHECK(ctx->pairLogE.ensure((size_t)PAIR_LUT * 8));
  HIPCHECK(ctx->pairCtab.ensure((size_t)PAIR_LUT * sizeof(CtrlEntry)));
  HIPCHECK(ctx->pairP2d.ensure((size_t)PT_N * PT_N * 4));
  HIPCHECK(ctx->dColl.ensure(64));
  HIPCHECK(ctx->dRisk.ensure(sizeof(RiskBuf)));
  HIPCHECK(ctx->dDeep.ensure(sizeof(DeepTab)));
  HIPCHECK(ctx->riskHost.ensure(sizeof(RiskBuf)));
  memset(ctx->riskHost.p, 0, 32);
  HIPCHECK(hipMemsetAsync(ctx->dRisk.p, 0, 32, ctx->stream));
  HIPCHECK(hipMemsetAsync(ctx->dDeep.p, 0, sizeof(DeepTab), ctx->stream));
  HIPCHECK(hipMemsetAsync(ctx->misc.p, 0, M_WORDS * 4, ctx->stream));
  HIPCHECK(hipMemsetAsync(ctx->dScal.p, 0, sizeof(Scalars), ctx->stream));
  HIPCHECK(hipMemsetAsync(ctx->dStatus.p, 0, 64, ctx->stream));
  HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tile<true, false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, TL_LDS * 4));
  {
    // persistent kernels: the grid must not exceed what is co-resident (look-back forward progress)
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, ctx->device));
    ctx->numCU = prop.multiProcessorCount;
    int nb = 0;
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_tile<true, false>, TL_NT, TL_LDS * 4));
    ctx->resTile = std::max(1, nb) * ctx->numCU;
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_tile<true, true>, TL_NT, TL_LDS_HALF * 4));
    ctx->resTileHalf = std::max(1, nb) * ctx->numCU;
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_tile_fast, 64, 0));
    ctx->resTileFast = std::max(1, std::min(nb, TF_WG_PER_CU)) * ctx->numCU;
    if (ctx->knob.debug)
      fprintf(stderr, "k_tile workgroups: half %d, wide %d, fast %d\n", ctx->resTileHalf, ctx->resTile, ctx->resTileFast);
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_scan_iv, STL_NT, 0));
    ctx->resSweep = std::max(1, std::min(nb, 4)) * ctx->numCU;
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_scan_iv_close_runs, STL_NT, 0));
    ctx->resScanRuns = std::max(1, std::min(nb, 4)) * ctx->numCU;
    // level 1 of the pair sort: its persistent grids are what the device keeps resident (a multiple of NXCD, so that a chunk's
    // XCD class is the one a grid of one workgroup per chunk gave it)
    int nbA = 1 << 30;
    for (auto k : {k_sort_a<false, false>, k_sort_a<false, true>, k_sort_a<true, false>, k_sort_a<true, true>}) {
      HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, S2_NT, 0));
      nbA = std::min(nbA, nb);
    }
    auto wholeXcds = [](int g) { return g > NXCD ? g - g % NXCD : std::max(1, g); };
    ctx->resSortA = wholeXcds(std::max(1, nbA) * ctx->numCU);
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_sort_b, S2_NT, 0));
    ctx->resSortB = wholeXcds(std::max(1, nb) * ctx->numCU);
    if (ctx->knob.debug) fprintf(stderr, "pair sort workgroups: k_sort_a %d, k_sort_b %d\n", ctx->resSortA, ctx->resSortB);
  }
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  return GX_OK;
}

void gx_destroy(gx_ctx* ctx) {
  if (!ctx) return;
  if (ctx->satChild) gx_destroy(ctx->satChild);   // (gx_saturation's child context)
  ctx->satChild = nullptr;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->comm) {
    if (const gxrccl::Api* api = gxrccl::load(nullptr)) (void)api->commDestroy(ctx->comm);
    ctx->comm = nullptr;
  }
  for (auto& ph : ctx->phases) {
    (void)hipEventDestroy(ph.a);
    (void)hipEventDestroy(ph.b);
  }
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  if (ctx->sideEv) (void)hipEventDestroy(ctx->sideEv);
  for (hipEvent_t e : ctx->evPool) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->stageFree) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->xcStageFree) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->gcStageFree) if (e) (void)hipEventDestroy(e);
  delete ctx;
}

const char* gx_last_error(const gx_ctx* ctx) { return ctx ? ctx->err.c_str() : ""; }

int gx_set_chroms(gx_ctx* ctx, int n, const uint32_t* len, const uint8_t* skip, const uint32_t* const* bed,
                  const int32_t* bed_len) {
  if (!ctx || n <= 0 || !len) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  repro_drop(ctx);
  if (ctx->satChild) sat_drop(ctx);   // (its table is the old one)
  ctx->nChrom = (u32)n;
  ctx->len.assign(len, len + n);
  ctx->skip.assign(n, 0);
  ctx->save.assign(n, 1);
  ctx->owned.assign(n, 1);
  ctx->bed.assign(n, {});
  ctx->bedGiven = false;
  for (int i = 0; i < n; i++) {
    ctx->skip[i] = skip && skip[i];
    if (bed && bed_len && bed_len[i] > 0 && !ctx->skip[i]) {
      ctx->bed[i].assign(bed[i], bed[i] + bed_len[i]);
      ctx->bedGiven = true;
    }
  }
  ctx->covDirty = true;
  ctx->profDirty = true;
  ctx->xcDirty = ctx->xcOn;
  ctx->gcDirty = ctx->gcOn;   // (the genome is laid out again, empty: its bases are pushed again)
  int rc = layout_tiles(ctx);
  if (rc) return rc;
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  return GX_OK;
}

int gx_set_collectives(gx_ctx* ctx, int rank, int world, gx_allreduce_i64_fn allreduce, void* user) {
  if (!ctx || world < 1 || rank < 0 || rank >= world) return GX_ERR_ORDER;
  if (ctx->comm && allreduce) {  // callbacks replace a communicator of gx_set_rccl
    if (const gxrccl::Api* api = gxrccl::load(nullptr)) (void)api->commDestroy(ctx->comm);
    ctx->comm = nullptr;
  }
  ctx->rank = rank;
  ctx->world = world;
  ctx->allreduce = allreduce;
  ctx->user = user;
  ctx->forceColl = ctx->knob.forceColl != 0;
  return GX_OK;
}

int gx_rccl_unique_id(void* out, size_t cap) {
  if (!out || cap < sizeof(ncclUniqueId)) return GX_ERR_ORDER;
  std::string err;
  const gxrccl::Api* api = gxrccl::load(&err);
  if (!api) {
    fprintf(stderr, "genrich_amd: %s\n", err.c_str());
    return GX_ERR_DEVICE;
  }
  ncclUniqueId id;
  if (api->getUniqueId(&id) != ncclSuccess) return GX_ERR_DEVICE;
  memcpy(out, &id, sizeof id);
  return GX_OK;
}

int gx_set_rccl(gx_ctx* ctx, int rank, int world, const void* unique_id) {
  if (!ctx || !unique_id || world < 1 || rank < 0 || rank >= world || world > 64) return GX_ERR_ORDER;
  const gxrccl::Api* api = gxrccl::load(&ctx->err);
  if (!api) return GX_ERR_DEVICE;
  HIPCHECK(hipSetDevice(ctx->device));
  if (ctx->comm) {
    (void)api->commDestroy(ctx->comm);
    ctx->comm = nullptr;
  }
  ncclUniqueId id;
  memcpy(&id, unique_id, sizeof id);
  ncclResult_t r = api->commInitRank(&ctx->comm, world, id, rank);
  if (r != ncclSuccess) {
    ctx->err = std::string("ncclCommInitRank: ") + api->getErrorString(r);
    ctx->comm = nullptr;
    return GX_ERR_DEVICE;
  }
  ctx->rank = rank;
  ctx->world = world;
  ctx->forceColl = ctx->knob.forceColl != 0;
  return GX_OK;
}

int gx_set_keep_pileups(gx_ctx* ctx, int keep) {
  if (!ctx) return GX_ERR_ORDER;
  ctx->keepPiles = keep != 0;
  return GX_OK;
}

int gx_set_owned(gx_ctx* ctx, const uint8_t* owned) {
  if (!ctx || !owned || ctx->nChrom == 0) return GX_ERR_ORDER;
  if (ctx->phase != 0 || ctx->sample != 0) return GX_ERR_ORDER;  // the tile space changes: between runs only
  repro_drop(ctx);
  if (ctx->satChild) sat_drop(ctx);   // (its mask is the old one)
  ctx->owned.assign(owned, owned + ctx->nChrom);
  ctx->covDirty = true;
  ctx->profDirty = true;
  ctx->xcDirty = ctx->xcOn;
  ctx->gcDirty = ctx->gcOn;   // (the genome is laid out again, empty: its bases are pushed again)
  int rc = layout_tiles(ctx);
  if (rc) return rc;
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  return GX_OK;
}

int gx_reset(gx_ctx* ctx) {
  if (!ctx) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  for (Pileup* P : {&ctx->expt, &ctx->ctrl}) {  // (samples stashed for a control merge give their buffers back)
    recycle(ctx, P->looseEnd); recycle(ctx, P->looseV); recycle(ctx, P->meta);
    P->inLoose = false;
  }
  for (auto& pa : ctx->reps) {
    recycle(ctx, pa.end); recycle(ctx, pa.p); recycle(ctx, pa.expt); recycle(ctx, pa.ctrl);
    recycle(ctx, pa.chromOff); recycle(ctx, pa.q); recycle(ctx, pa.tileOff); recycle(ctx, pa.dPresent);
    recycle(ctx, pa.chromLooseOff); recycle(ctx, pa.keptV); recycle(ctx, pa.keptMeta);
  }
  ctx->reps.clear();
  ctx->pilesMade = false;
  ctx->sample = 0;
  ctx->phase = 0;
  ctx->finalIdx = -1;
  ctx->segs.clear();
  ctx->unpackUsed = 0;
  ctx->evChunkIdx = ctx->evChunkFill = ctx->evPoolUsed = 0;
  ctx->nHostPeaks = 0;
  drop_kept(ctx);   // (the switch itself stays: gx_set_count_in_peaks)
  drop_coverage(ctx);   // (... and gx_set_coverage_bins')
  drop_profile(ctx);    // (... and gx_set_profile's)
  drop_depth(ctx);      // (... and gx_set_depth_hist's)
  drop_xcor(ctx);       // (... and gx_set_xcor's)
  drop_gcbias(ctx);     // (gx_gc_bias' results; the genome stays)
  drop_motifs(ctx);     // (gx_motif_scan_peaks' results; the motifs stay)
  drop_kmers(ctx);      // (gx_kmer_count_peaks' results)
  ctx->gramUsed = false;
  ctx->fpUsed = false;
  ctx->rankUsed = false;
  ctx->cpx.clear();     // (the buffers stay with the context)
  ctx->cpxReady = ctx->cpxUsed = false;
  ctx->ivs.clear();
  ctx->ivsReady = ctx->ivsUsed = false;
  ctx->psigReady = false;   // (gx_peak_signal's records go with the peaks; the buffers stay)
  ctx->sumRes.clear();      // (gx_peak_summits' summits too)
  ctx->sumReady = false;
  repro_drop(ctx);          // (gx_reproducibility's calls and k_sub_split's bit)
  if (ctx->satChild || ctx->subUsed || !ctx->subBufs.empty()) sat_drop(ctx);   // (the child context goes; the buffers stay with the pool)
  ctx->peaksReady = false;
  ctx->specRuns.valid = false;
  ctx->called.ran.overlap = false;
  if (ctx->statusSeen) {  // (a clean run leaves the status words at zero: no fill launch)
    HIPCHECK(hipMemsetAsync(ctx->dStatus.p, 0, 64, ctx->stream));
    ctx->statusSeen = 0;
  }
  return GX_OK;
}

int gx_sample_begin(gx_ctx* ctx, int is_ctrl, const uint8_t* save) {
  if (!ctx || ctx->nChrom == 0) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  ctx->specRuns.valid = false;   // (a control or a further replicate: the sweep will not be the one the run pass was launched for)
  if (!is_ctrl) {
    if (ctx->phase != 0) return GX_ERR_ORDER;
    ctx->peaksReady = ctx->countsReady = ctx->psigReady = ctx->sumReady = ctx->motReady = ctx->kmReady = false;
    // (a further replicate: the previous one's loose slots, tile tables and p(V) table are about to be reused)
    for (size_t r = 0; r < ctx->reps.size(); r++)
      if (ctx->reps[r].loose || ctx->reps[r].pilesPending)
        if (int rc = keep_loose_for_piles(ctx, (int)r)) return rc;
    for (u32 i = 0; i < ctx->nChrom; i++) ctx->save[i] = save ? (save[i] != 0) : 1;
    int rc = upload_chroms(ctx, false);
    if (rc) return rc;
    uint64_t g = ctx->par.genome_len ? ctx->par.genome_len : genome_len_for(ctx, ctx->save);
    if (!g) {
      ctx->err = "No analyzable genome (length=0)";
      return GX_ERR_GEN;  // calcLambda 1828
    }
    Scalars z{};
    z.genomeLen = g;
    ctx->hScal = z;
    // (the device's copy is cleared by the first launch of the build: k_build_init)
    ctx->beginPending = true;
    ctx->beginGenome = (u64)g;
    ctx->nPhases = 0;
    ctx->phase = 1;
  } else {
    if (ctx->phase != 2) return GX_ERR_ORDER;
    int rc = stash_or_pack(ctx, ctx->expt);  // the control's tiles are about to be built: the treatment steps aside
    if (rc) return rc;
    ctx->phase = 3;
  }
  ctx->segs.clear();
  ctx->unpackUsed = 0;
  ctx->evChunkIdx = ctx->evChunkFill = ctx->evPoolUsed = 0;  // (the previous sample's uploads were consumed: gx_sample_end synchronised)
  ctx->satDone = false;
  ctx->satDropped = 0;
  if (ctx->xcOn)
    if (int rc = xc_begin(ctx)) return rc;
  return GX_OK;
}

namespace {

constexpr size_t EV_CHUNK = (size_t)1 << 22;   // events per device chunk (64 MiB)
constexpr size_t EV_STAGE = (size_t)1 << 20;   // events per pinned staging buffer (16 MiB)

hipEvent_t ready_event(gx_ctx* ctx) {
  if (ctx->evPoolUsed == ctx->evPool.size()) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    ctx->evPool.push_back(e);
  }
  return ctx->evPool[ctx->evPoolUsed++];
}

// Host events -> the library's device chunks, by asynchronous copies on the side stream.  `pinned`: the
// caller's memory is page-locked and stays untouched until gx_sample_end, so it is the copy's source itself;
// otherwise the events go through two pinned staging buffers (the caller's buffer is free on return, and the
// host keeps parsing while a buffer is in flight).  Nothing here waits for a copy to arrive: every piece
// carries an event that the main stream waits for before the kernel that reads it (build_pileup).
// (`esz`: 16, gx_event, or 8, gx_event8: the chunks are filled in 16-byte units either way, so every piece starts on a 16-byte
// boundary -- k_sort_a<.., PACKED> reads two packed events per load -- and a piece with an odd count leaves 8 bytes unused)
int push_host(gx_ctx* ctx, const void* events_, size_t n, bool pinned, size_t esz) {
  const char* events = static_cast<const char*>(events_);
  const size_t per16 = sizeof(gx_event) / esz;   // events per 16-byte unit
  while (n) {
    if (ctx->evChunkIdx == ctx->evChunks.size()) ctx->evChunks.emplace_back();
    DevBuf& chunk = ctx->evChunks[ctx->evChunkIdx];
    HIPCHECK(chunk.ensure(EV_CHUNK * sizeof(gx_event)));
    size_t take = std::min(n, (EV_CHUNK - ctx->evChunkFill) * per16);
    if (!pinned) take = std::min(take, EV_STAGE * per16);
    char* dst = chunk.as<char>() + ctx->evChunkFill * sizeof(gx_event);
    const char* src = events;
    if (!pinned) {
      const int k = ctx->stageNext;
      ctx->stageNext ^= 1;
      HIPCHECK(ctx->stage[k].ensure(EV_STAGE * sizeof(gx_event)));
      if (!ctx->stageFree[k]) HIPCHECK(hipEventCreateWithFlags(&ctx->stageFree[k], hipEventDisableTiming));
      else HIPCHECK(hipEventSynchronize(ctx->stageFree[k]));  // its previous upload has left the buffer
      memcpy(ctx->stage[k].p, events, take * esz);
      src = static_cast<const char*>(ctx->stage[k].p);
      HIPCHECK(hipMemcpyAsync(dst, src, take * esz, hipMemcpyHostToDevice, ctx->side));
      HIPCHECK(hipEventRecord(ctx->stageFree[k], ctx->side));
    } else
      HIPCHECK(hipMemcpyAsync(dst, src, take * esz, hipMemcpyHostToDevice, ctx->side));
    hipEvent_t ev = ready_event(ctx);
    if (!ev) { ctx->err = "hipEventCreate failed"; return GX_ERR_DEVICE; }
    HIPCHECK(hipEventRecord(ev, ctx->side));
    ctx->segs.push_back({reinterpret_cast<const gx_event*>(dst), take, ev, esz != sizeof(gx_event)});
    ctx->evChunkFill += (take + per16 - 1) / per16;
    if (ctx->evChunkFill == EV_CHUNK) { ctx->evChunkIdx++; ctx->evChunkFill = 0; }
    events += take * esz;
    n -= take;
  }
  return GX_OK;
}

}  // namespace

int gx_push_events(gx_ctx* ctx, const gx_event* events, size_t n) {
  if (!ctx || (ctx->phase != 1 && ctx->phase != 3)) return GX_ERR_ORDER;
  if (!n) return GX_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  return push_host(ctx, events, n, false, sizeof(gx_event));
}

int gx_push_events_pinned(gx_ctx* ctx, const gx_event* events, size_t n) {
  if (!ctx || (ctx->phase != 1 && ctx->phase != 3)) return GX_ERR_ORDER;
  if (!n) return GX_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  return push_host(ctx, events, n, true, sizeof(gx_event));
}

int gx_push_events_packed(gx_ctx* ctx, const gx_event8* events, size_t n, int where) {
  if (!ctx || (ctx->phase != 1 && ctx->phase != 3) || where < 0 || where > 2) return GX_ERR_ORDER;
  if (!n) return GX_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  if (where == GX_EVENTS_DEVICE) {
    // (used in place; k_sort_a reads two records per 16-byte load: a buffer that does not start on a 16-byte boundary, or an odd
    // count at its end, goes through the 16-byte form instead -- unpack_segs)
    ctx->segs.push_back({reinterpret_cast<const gx_event*>(events), n, nullptr, true});
    return GX_OK;
  }
  return push_host(ctx, events, n, where == GX_EVENTS_PINNED, sizeof(gx_event8));
}

int gx_event8_pack(const gx_event* in, gx_event8* out) {
  if (!in || !out) return 0;
  const uint32_t len = in->end - in->start;
  uint32_t cls = 8;
  for (uint32_t k = 0; k < 8; k++)
    if ((uint32_t)((0xA8654321u >> (4u * k)) & 15u) == in->count) cls = k;
  if (in->end < in->start || len >= 0xFFFFu || cls == 8 || in->chrom >= (1u << 13)) return 0;
  out->start = in->start;
  out->lcc = len | (cls << 16) | (in->chrom << 19);
  return 1;
}

long long gx_filter_saturation(const gx_event* events, size_t n, int n_chrom, const uint32_t* len, uint8_t* keep) {
  if ((!events && n) || (!keep && n) || n_chrom < 0 || (!len && n_chrom)) return GX_ERR_ORDER;
  return gxsat::filter(events, n, n_chrom, len, keep);
}

int gx_push_events_device(gx_ctx* ctx, const gx_event* d_events, size_t n) {
  if (!ctx || (ctx->phase != 1 && ctx->phase != 3)) return GX_ERR_ORDER;
  if (n) ctx->segs.push_back({d_events, n, nullptr});
  return GX_OK;
}

int gx_sample_end(gx_ctx* ctx, double* frag_len, float* lambda, float* factor) {
  if (!ctx) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  if (ctx->phase == 1) {
    int rc = close_sample(ctx, ctx->expt, 0);
    if (rc) return rc;
    ctx->phase = 2;
  } else if (ctx->phase == 3) {
    int rc = close_sample(ctx, ctx->ctrl, 1);
    if (rc) return rc;
    ctx->phase = 4;
  } else
    return GX_ERR_ORDER;
  if (ctx->covW)
    if (int rc = cov_sample(ctx, ctx->phase == 4)) return rc;
  if (ctx->depthOn)
    if (int rc = depth_sample(ctx, ctx->phase == 4)) return rc;
  if (ctx->xcOn)
    if (int rc = xc_sample(ctx, ctx->phase == 4)) return rc;
  if (!ctx->profAnchors.empty())
    if (int rc = prof_sample(ctx, ctx->phase == 4)) return rc;
  if (ctx->countOn) keep_sample(ctx, ctx->phase == 4);
  if (frag_len) *frag_len = ctx->hScal.fragLen;
  if (lambda) *lambda = ctx->hScal.lambda;
  if (factor) *factor = ctx->hScal.factor;
  return GX_OK;
}

int gx_expect_fractional(gx_ctx* ctx, int on) {
  if (!ctx) return GX_ERR_ORDER;
  // (a hint selects kernels; what the library has learned from a sample by itself -- sawFrac -- is not the hint's to clear)
  ctx->fracHint = on != 0;
  return GX_OK;
}

int gx_set_knob(gx_ctx* ctx, const char* name, const char* value) {
  if (!ctx || !name) return GX_ERR_ORDER;
  // (GX_BH_CAPLOG, GX_PT_JMAX and GX_SBSHIFT size tables when the context and its tile layout are made: on a live context
  // they would change nothing, so they are refused instead of accepted without effect)
  for (const char* fixed : {"GX_BH_CAPLOG", "GX_PT_JMAX", "GX_SBSHIFT"})
    if (!strcmp(name, fixed)) {
      ctx->err = std::string(name) + " is read when the context is made (environment); it cannot change afterwards";
      return GX_ERR_ORDER;
    }
  if (!set_knob(ctx->knob, name, value)) {
    ctx->err = std::string("unknown switch ") + name;
    return GX_ERR_ORDER;
  }
  ctx->forceColl = ctx->knob.forceColl != 0;
  return GX_OK;
}

int gx_dups_first(gx_ctx* ctx, const gx_dup_key* keys, const uint8_t* multi, size_t n, uint32_t* owner) {
  // (the table has 2^k >= 2 n slots addressed by 32-bit indices: n <= 2^30)
  if (!ctx || (n && (!keys || !multi || !owner)) || n > ((size_t)1 << 30)) return GX_ERR_ORDER;
  if (!n) return GX_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const u32 cap = dup_capacity(n);
  DevBuf dKeys, dMulti, dOwner, dTab;
  HIPCHECK(dKeys.ensure(n * 16));
  HIPCHECK(dMulti.ensure(n + 16));
  HIPCHECK(dOwner.ensure(n * 4));
  HIPCHECK(dTab.ensure((size_t)cap * 12));
  HIPCHECK(hipMemcpyAsync(dKeys.p, keys, n * 16, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(dMulti.p, multi, n, hipMemcpyHostToDevice, s));
  DupTab T{dTab.as<u32>(), dTab.as<u32>() + cap, dTab.as<u32>() + 2 * (size_t)cap, cap - 1};
  HIPCHECK(hipMemsetAsync(T.rep, 0xFF, (size_t)cap * 8, s));   // rep = free, first = "no index yet"
  HIPCHECK(hipMemsetAsync(T.multi, 0, (size_t)cap * 4, s));
  const u32 blocks = (u32)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 8192));
  hipLaunchKernelGGL(k_dups_insert, dim3(blocks), dim3(256), 0, s, dKeys.as<uint4>(), (const uint8_t*)dMulti.as<uint8_t>(), (u32)n, T);
  hipLaunchKernelGGL(k_dups_lookup, dim3(blocks), dim3(256), 0, s, dKeys.as<uint4>(), (u32)n, T, dOwner.as<u32>());
  HIPCHECK(hipMemcpyAsync(owner, dOwner.p, n * 4, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  HIPCHECK(hipGetLastError());
  return GX_OK;
}

int gx_dups_geometry(const gx_dup_key* keys, size_t n, uint32_t* capacity, uint32_t* home) {
  if (n > ((size_t)1 << 30) || (n && home && !keys)) return GX_ERR_ORDER;
  const u32 cap = dup_capacity(n);
  if (capacity) *capacity = cap;
  if (home)
    for (size_t i = 0; i < n; i++) home[i] = dup_hash(make_uint4(keys[i].w[0], keys[i].w[1], keys[i].w[2], keys[i].w[3])) & (cap - 1);
  return GX_OK;
}

int gx_saturation_dropped(gx_ctx* ctx, long long* n) {
  if (!ctx || !n) return GX_ERR_ORDER;
  *n = ctx->satDropped;
  return GX_OK;
}

int gx_window_net(gx_ctx* ctx, uint32_t chrom, uint32_t pos0, uint32_t n, long long* net) {
  if (!ctx || (ctx->phase != 1 && ctx->phase != 3) || !net || !n || n > (1u << 16) || chrom >= ctx->nChrom) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (int rc__ = unpack_segs(ctx, true)) return rc__;
  DevBuf dNet;
  HIPCHECK(dNet.ensure((size_t)n * 8));
  HIPCHECK(hipMemsetAsync(dNet.p, 0, (size_t)n * 8, s));
  for (auto& sg : ctx->segs) {
    if (!sg.n) continue;
    if (sg.ready) HIPCHECK(hipStreamWaitEvent(s, sg.ready, 0));  // (its upload, on the side stream)
    const u32 blocks = (u32)std::min<size_t>((sg.n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_window_net, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const uint4*>(sg.p), sg.n, chrom, ctx->len[chrom],
                       pos0, n, dNet.as<unsigned long long>());
  }
  HIPCHECK(hipMemcpyAsync(net, dNet.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  HIPCHECK(hipGetLastError());
  return GX_OK;
}

int gx_sample_no_control(gx_ctx* ctx, float* lambda) {
  if (!ctx || ctx->phase != 2) return GX_ERR_ORDER;
  if (lambda) *lambda = ctx->hScal.lambda;  // computed with fragLen (calcLambda 1831)
  ctx->phase = 5;
  return GX_OK;
}

int gx_pvalues(gx_ctx* ctx) {
  if (!ctx || (ctx->phase != 4 && ctx->phase != 5)) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  PArray pa;
  pa.present.assign(ctx->nChrom, 0);
  for (u32 i = 0; i < ctx->nChrom; i++) pa.present[i] = !ctx->skip[i] && ctx->save[i];
  if (ctx->phase == 5) {
    // no control: the p-intervals are the treatment intervals, and they stay where the tile kernel left them
    // (loose slots) until somebody needs the tight table: gx_find_peaks on a single sample with -p does not
    pa.n = ctx->expt.nIv;
    pa.chromOff = std::move(ctx->expt.chromIvOff);
    pa.tileOff = std::move(ctx->expt.tileIvOff);
    pa.ctrlIsConst = !ctx->hasBed;
    pa.ctrlConst = ctx->hScal.lambda;
    pa.loose = true;
    // (the tile stage wrote the sweep's significance bits, in loose-slot index space: LooseCtl)
    pa.looseSweep = ctx->looseOk && (!ctx->par.qval_opt || (q_loose_may(ctx) && ctx->built.wantLate)) && !ctx->knob.noLoose;   // (-q: plan_call's LOOSE_Q)
    pa.latePending = pa.looseSweep && ctx->built.wantLate;   // (its bits are still to be written: k_loose_late, by gx_find_peaks)
    pa.looseStride = ctx->looseStride;
    if (pa.looseSweep) pa.chromLooseOff = std::move(ctx->chromLooseOff);
    ctx->looseOk = false;
    ctx->reps.push_back(std::move(pa));
    ctx->sample++;
    ctx->phase = 0;
    return GX_OK;
  } else {
    if (int rc = merge_with_control(ctx, pa)) return rc;
  }
  ctx->reps.push_back(std::move(pa));
  ctx->sample++;
  ctx->phase = 0;
  return GX_OK;
}

int gx_find_peaks(gx_ctx* ctx, size_t* n_peaks, uint64_t* genome_len, uint64_t* peak_bp) {
  if (!ctx || ctx->phase != 0 || ctx->sample < 1) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  ctx->peaksReady = ctx->countsReady = ctx->psigReady = ctx->sumReady = ctx->motReady = ctx->kmReady = false;
  const CallPlan& P = ctx->called;
  u32 nPeaks = 0;
  // (at most two plans: -q on the loose slots may be called off by the device, and the call is then planned again without it)
  for (int attempt = 0;; attempt++) {
    if (int rc = plan_call(ctx)) return rc;
    if (int rc = call_tables(ctx, P)) return rc;
    call_scalars(ctx, P);
    if (int rc = call_bh(ctx, P)) return rc;
    phase_begin(ctx, "sweep");
    SweepSrc src;
    if (int rc = call_sweep_source(ctx, P, src)) return rc;
    bool synced = false;
    const int rcSweep = run_sweep(ctx, src, &nPeaks, &synced);
    phase_end(ctx);
    if (attempt == 0 && P.walk == CallPlan::LOOSE_Q && synced && (ctx->mail->status & ST_Q_LOOSE)) {
      // q turned out to be no threshold on the pileup (a table p(V) that is not monotone): once more, on the tight table -- and from now on
      HIPCHECK(hipMemsetAsync(ctx->dStatus.p, 0, 4, ctx->stream));
      ctx->qLooseBad = true;
      continue;
    }
    if (rcSweep) return rcSweep;
    break;
  }
  ctx->peaksReady = true;
  if (n_peaks) *n_peaks = nPeaks;
  if (genome_len) *genome_len = P.g;
  if (peak_bp) *peak_bp = ctx->peakBP;
  return GX_OK;
}

int gx_peak_count(gx_ctx* ctx, size_t* n) {
  if (!ctx || !n) return GX_ERR_ORDER;
  *n = ctx->nHostPeaks;
  return GX_OK;
}

int gx_get_peaks(gx_ctx* ctx, gx_peak* out, size_t cap) {
  if (!ctx || !out) return GX_ERR_ORDER;
  size_t n = std::min(cap, ctx->nHostPeaks);
  if (n) memcpy(out, ctx->hPeaks.p, n * sizeof(gx_peak));
  return GX_OK;
}

static const PArray* which_array(gx_ctx* ctx, int which, int chrom, u32* lo, u32* hi) {
  if (chrom < 0 || (u32)chrom >= ctx->nChrom) return nullptr;
  int w = which == GX_IV_FINAL ? ctx->finalIdx : which;
  if (w < 0 || w >= (int)ctx->reps.size()) return nullptr;
  if (ctx->reps[w].loose && materialize_rep(ctx, w) != GX_OK) return nullptr;
  const PArray& pa = ctx->reps[w];
  if (!pa.present[chrom]) return nullptr;
  u32 off[2];
  if (hipMemcpy(off, pa.chromOff.as<u32>() + chrom, 8, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
  *lo = off[0];
  *hi = off[1];
  return &pa;
}

int gx_interval_count(gx_ctx* ctx, int which, int chrom, size_t* n_iv) {
  if (!ctx || !n_iv) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  u32 lo = 0, hi = 0;
  const PArray* pa = which_array(ctx, which, chrom, &lo, &hi);
  *n_iv = pa ? hi - lo : 0;
  return GX_OK;
}

int gx_get_intervals(gx_ctx* ctx, int which, int chrom, size_t cap, uint32_t* end, float* expt, float* ctrl, float* p,
                     float* q) {
  if (!ctx) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  u32 lo = 0, hi = 0;
  const PArray* pa = which_array(ctx, which, chrom, &lo, &hi);
  if (!pa) return GX_OK;
  size_t n = std::min<size_t>(cap, hi - lo);
  if ((expt || ctrl) && pa->pilesPending) {
    const int w = which == GX_IV_FINAL ? ctx->finalIdx : which;
    if (int rc = ensure_piles(ctx, w)) return rc;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
  }
  if ((expt || ctrl) && pa->pilesDropped) {
    ctx->err = "the pileup values were not kept (gx_set_keep_pileups)";
    return GX_ERR_ORDER;
  }
  if (!n) return GX_OK;
  if (end) HIPCHECK(hipMemcpy(end, pa->end.as<u32>() + lo, n * 4, hipMemcpyDeviceToHost));
  if (p) HIPCHECK(hipMemcpy(p, pa->p.as<float>() + lo, n * 4, hipMemcpyDeviceToHost));
  if (expt) {
    if (pa->hasPiles) HIPCHECK(hipMemcpy(expt, pa->expt.as<float>() + lo, n * 4, hipMemcpyDeviceToHost));
    else std::fill(expt, expt + n, 0.0f);
  }
  if (ctrl) {
    if (pa->hasPiles && !pa->ctrlIsConst) HIPCHECK(hipMemcpy(ctrl, pa->ctrl.as<float>() + lo, n * 4, hipMemcpyDeviceToHost));
    else std::fill(ctrl, ctrl + n, pa->ctrlIsConst ? pa->ctrlConst : 0.0f);
  }
  if (q) {
    if ((pa->q.p || pa->qLazy) && ctx->par.qval_opt) {
      const int w = which == GX_IV_FINAL ? ctx->finalIdx : which;
      if (int rc = ensure_q(ctx, ctx->reps[w], w)) return rc;
      HIPCHECK(hipStreamSynchronize(ctx->stream));
      HIPCHECK(hipMemcpy(q, pa->q.as<float>() + lo, n * 4, hipMemcpyDeviceToHost));
    }
    if (!((pa->q.p || pa->qLazy) && ctx->par.qval_opt)) std::fill(q, q + n, GX_SKIP);
  }
  return GX_OK;
}

int gx_selftest2(gx_ctx* ctx, int what, const float* a, const float* b, float* out, double* out_double, size_t n,
                 size_t* n_risky) {
  if (!ctx || !a || !out || !n || n > 0xFFFFFFFFull) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  DevBuf da, db, dout, ddbl;
  HIPCHECK(da.ensure(n * 4));
  HIPCHECK(db.ensure(n * 4));
  HIPCHECK(dout.ensure(n * 4));
  if (out_double) HIPCHECK(ddbl.ensure(n * 8));
  HIPCHECK(hipMemcpy(da.p, a, n * 4, hipMemcpyHostToDevice));
  if (b) HIPCHECK(hipMemcpy(db.p, b, n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest, dim3(1024), dim3(256), 0, ctx->stream, what, da.as<float>(), db.as<float>(),
                     dout.as<float>(), ddbl.as<double>(), (u32)n, ctx->dRisk.as<RiskBuf>());
  if (int rc__ = dbg_sync(ctx, "k_selftest")) return rc__;
  if (int rc__ = mail_sync(ctx, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc__;
  if (n_risky) *n_risky = static_cast<RiskBuf*>(ctx->riskHost.p)->count;
  RiskTargets T{};
  T.selfOut = dout.as<float>();
  if (int rc__ = risk_apply(ctx, T, RiskHostIn{a, b})) return rc__;
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  HIPCHECK(hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost));
  if (out_double) HIPCHECK(hipMemcpy(out_double, ddbl.p, n * 8, hipMemcpyDeviceToHost));
  return GX_OK;
}

int gx_selftest(gx_ctx* ctx, int what, const float* a, const float* b, float* out, size_t n) {
  return gx_selftest2(ctx, what, a, b, out, nullptr, n, nullptr);
}

// the same scalar routines compiled for the host (what 1: calcPval, 3: multPval's tail): what the library
// evaluates risky values with, i.e. with this machine's libm; no context, no device
int gx_selftest_host(int what, const float* a, const float* b, float* out, double* out_double, size_t n) {
  if (!a || !b || !out || (what != 1 && what != 3 && what != 4)) return GX_ERR_ORDER;
  for (size_t i = 0; i < n; i++) {
    bool rk = false;
    double d = 0.0;
    if (what == 1) {
      out[i] = calc_pval(a[i], b[i], &rk);
      if (a[i] > 0.0f && b[i] > 0.0f) {
        double ml, sl;
        lnorm_params(b[i], &ml, &sl);
        d = pval_double(a[i], log((double)a[i]), ml, sl);
      }
    } else if (what == 3) {
      out[i] = fisher_combine((double)a[i], (int)b[i], &rk);
      if ((int)b[i] > 2 && a[i] != 0.0f) d = fisher_double((double)a[i], (int)b[i]);
    } else {   // (4: the closed form, host build -- NOT what the library's host side ever rounds: a check of the formula itself)
      out[i] = fisher_fast((double)a[i], (int)b[i], &rk);
      if ((int)b[i] > 2 && a[i] != 0.0f) d = fisher_fast_double((double)a[i], (int)b[i]);
    }
    if (out_double) out_double[i] = d;
  }
  return GX_OK;
}

int gx_total_intervals(gx_ctx* ctx, int which, size_t* n_iv) {
  if (!ctx || !n_iv) return GX_ERR_ORDER;
  int w = which == GX_IV_FINAL ? ctx->finalIdx : which;
  if (w < 0 || w >= (int)ctx->reps.size()) return GX_ERR_ORDER;
  *n_iv = ctx->reps[w].n;
  return GX_OK;
}

int gx_set_phase_filter(gx_ctx* ctx, const char* name) {
  if (!ctx || !name) return GX_ERR_ORDER;
  ctx->phaseFilter = name;
  ctx->phaseLevel = 1;
  return GX_OK;
}

int gx_rccl_nranks(gx_ctx* ctx, int* n) {
  if (!ctx || !n) return GX_ERR_ORDER;
  *n = 0;
  if (ctx->comm) {
    const gxrccl::Api* api = gxrccl::load(nullptr);
    if (api && api->commCount && api->commCount(ctx->comm, n) != ncclSuccess) *n = 0;
  }
  return GX_OK;
}

int gx_path_info(gx_ctx* ctx, unsigned* flags) {
  if (!ctx || !flags) return GX_ERR_ORDER;
  // the calling half's bits from the last call's plan and what its run told; the build half's from the last build's plan
  const CallPlan& C = ctx->called;
  const bool dense = C.exchange == CallPlan::X_DENSE && !C.ran.denseFellBack;
  const bool range = C.exchange == CallPlan::X_RANGE || (C.exchange == CallPlan::X_DENSE && C.ran.denseFellBack);
  const bool packHist = C.bh == CallPlan::BH_SMALL || (C.bh == CallPlan::BH_FROM_DENSE && !C.ran.tableGrew);
  *flags = (ctx->built.fused ? GX_PATH_FUSED : 0u) | (ctx->built.fused && ctx->built.pairs ? GX_PATH_PAIRS : 0u) | (dense ? GX_PATH_DENSE_BH : 0u) | (range ? GX_PATH_RANGE_BH : 0u) | (C.looseSwept() ? GX_PATH_LOOSE_SWEEP : 0u) |
           (ctx->fellBack ? GX_PATH_FELL_BACK : 0u) | (ctx->ptGrew ? GX_PATH_PT_GREW : 0u) | (ctx->built.fused && ctx->built.fracPairs ? GX_PATH_FRAC_PAIRS : 0u) |
           (ctx->pilesMade ? GX_PATH_PILES_MADE : 0u) | (ctx->packedUsed ? GX_PATH_PACKED : 0u) | (ctx->mergePUsed ? GX_PATH_MERGE_P : 0u) |
           (packHist ? GX_PATH_PACK_HIST : 0u) | (C.lazyQ ? GX_PATH_LAZY_Q : 0u) | (C.looseSwept() && C.lateBits() ? GX_PATH_LATE_LOOSE : 0u) | (C.walk == CallPlan::LOOSE_Q ? GX_PATH_Q_LOOSE : 0u) |
           (ctx->countOn && !ctx->kept.empty() ? GX_PATH_COUNTS : 0u) | (ctx->regionsReady ? GX_PATH_REGION_COUNTS : 0u) |
           (ctx->covW && !ctx->cov.empty() ? GX_PATH_COVERAGE : 0u) | (!ctx->prof.empty() ? GX_PATH_PROFILE : 0u) |
           (ctx->gramUsed ? GX_PATH_GRAM : 0u) | (ctx->fpUsed ? GX_PATH_FINGERPRINT : 0u) | (ctx->rankUsed ? GX_PATH_SPEARMAN : 0u) |
           (ctx->cpxUsed ? GX_PATH_COMPLEXITY : 0u) | (ctx->subUsed ? GX_PATH_SATURATION : 0u) | (ctx->depthUsed ? GX_PATH_DEPTH : 0u) | (ctx->ivsUsed ? GX_PATH_IVSTAT : 0u) |
           (ctx->xcUsed ? GX_PATH_XCOR : 0u) | (ctx->gcUsed ? GX_PATH_GC : 0u) | (ctx->motUsed ? GX_PATH_MOTIFS : 0u) | (ctx->kmUsed ? GX_PATH_KMERS : 0u) | (ctx->splitUsed ? GX_PATH_SPLIT : 0u) | (C.looseSwept() && C.ran.overlap ? GX_PATH_SWEEP_OVERLAP : 0u);
  return GX_OK;
}

int gx_set_count_in_peaks(gx_ctx* ctx, int on) {
  if (!ctx || ctx->phase != 0 || ctx->sample != 0) return GX_ERR_ORDER;   // idle: after gx_create / gx_reset, before a sample
  ctx->countOn = on != 0;
  if (!ctx->countOn) drop_kept(ctx);
  return GX_OK;
}

int gx_count_in_peaks(gx_ctx* ctx, int* n_samples) {
  if (!ctx || !ctx->countOn || !ctx->peaksReady || ctx->phase != 0) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  if (int rc = count_in_peaks(ctx)) return rc;
  if (n_samples) *n_samples = (int)ctx->kept.size();
  return GX_OK;
}

int gx_get_peak_counts(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, int64_t* count120, size_t cap, int64_t* total120,
                       int64_t* in_peaks120) {
  if (!ctx || !ctx->countsReady || sample < 0 || (size_t)sample >= ctx->kept.size() || (cap && !count120)) return GX_ERR_ORDER;
  return give_counts(ctx, ctx->cntHost, ctx->cntPk, sample, rep, is_ctrl, count120, cap, total120, in_peaks120);
}

int gx_count_in_regions(gx_ctx* ctx, const gx_region* regions, size_t n, int* n_samples) {
  if (!ctx || !ctx->countOn || ctx->phase == 1 || ctx->phase == 3 || (n && !regions)) return GX_ERR_ORDER;
  for (size_t k = 0; k < n; k++)
    if (regions[k].start >= regions[k].end) {
      ctx->err = "a region with start >= end";
      return GX_ERR_ORDER;
    }
  HIPCHECK(hipSetDevice(ctx->device));
  ctx->regionsReady = false;
  if (int rc = count_in_regions(ctx, regions, n)) return rc;
  ctx->regionsReady = true;
  if (n_samples) *n_samples = (int)ctx->regSamples;
  return GX_OK;
}

int gx_get_region_counts(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, int64_t* count120, size_t cap, int64_t* total120,
                         int64_t* in_regions120) {
  if (!ctx || !ctx->regionsReady || sample < 0 || (u32)sample >= ctx->regSamples || (cap && !count120)) return GX_ERR_ORDER;
  return give_counts(ctx, ctx->regHost, ctx->regN, sample, rep, is_ctrl, count120, cap, total120, in_regions120);
}

int gx_set_coverage_bins(gx_ctx* ctx, uint32_t bin_size) {
  if (!ctx || ctx->nChrom == 0 || ctx->phase != 0 || ctx->sample != 0) return GX_ERR_ORDER;   // idle, and the table is known
  if (bin_size > COV_MAX_W) {
    ctx->err = "coverage bins of more than 2^20 bases";
    return GX_ERR_ORDER;
  }
  HIPCHECK(hipSetDevice(ctx->device));
  const u32 before = ctx->covW;
  drop_coverage(ctx);
  if (bin_size == before && !ctx->covDirty) return GX_OK;   // (the layout on the device is this one already)
  ctx->covW = bin_size;
  ctx->covDirty = true;
  if (!bin_size) return GX_OK;
  if (int rc = cov_layout(ctx)) {
    ctx->covW = before;
    ctx->covDirty = true;
    return rc;
  }
  return GX_OK;
}

int gx_coverage_samples(gx_ctx* ctx, int* n_samples) {
  if (!ctx || !n_samples) return GX_ERR_ORDER;
  *n_samples = (int)ctx->cov.size();
  return GX_OK;
}

int gx_coverage_layout(gx_ctx* ctx, int chrom, uint32_t* bin_size, uint32_t* len) {
  if (!ctx || chrom < 0 || (u32)chrom >= ctx->nChrom) return GX_ERR_ORDER;
  if (bin_size) *bin_size = ctx->covW;
  if (len) *len = ctx->len[chrom];
  return GX_OK;
}

int gx_coverage_bin_count(gx_ctx* ctx, int chrom, size_t* n_bins) {
  if (!ctx || !n_bins || chrom < 0 || (u32)chrom >= ctx->nChrom) return GX_ERR_ORDER;
  *n_bins = 0;
  if (!ctx->covW) return GX_OK;
  if (ctx->covDirty)
    if (int rc = cov_layout(ctx)) return rc;
  *n_bins = ctx->covOff[chrom + 1] - ctx->covOff[chrom];
  return GX_OK;
}

int gx_get_coverage(gx_ctx* ctx, int sample, int chrom, int* rep, int* is_ctrl, int64_t* sum120, size_t cap) {
  if (!ctx || ctx->phase == 1 || ctx->phase == 3 || sample < 0 || (size_t)sample >= ctx->cov.size() || chrom < 0 ||
      (u32)chrom >= ctx->nChrom || (cap && !sum120))
    return GX_ERR_ORDER;
  const gx_ctx::CovSample& c = ctx->cov[sample];
  if (rep) *rep = c.rep;
  if (is_ctrl) *is_ctrl = c.ctrl ? 1 : 0;
  const size_t n = std::min(cap, ctx->covOff[chrom + 1] - ctx->covOff[chrom]);
  if (!n) return GX_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  HIPCHECK(hipMemcpyAsync(sum120, c.bins.as<int64_t>() + ctx->covOff[chrom], n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  return GX_OK;
}

int gx_set_depth_hist(gx_ctx* ctx, int on) {
  if (!ctx || ctx->nChrom == 0 || ctx->phase != 0 || ctx->sample != 0) return GX_ERR_ORDER;   // idle, and the table is known
  ctx->depthOn = on != 0;
  drop_depth(ctx);
  return GX_OK;
}

int gx_depth_samples(gx_ctx* ctx, int* n_samples) {
  if (!ctx || !n_samples) return GX_ERR_ORDER;
  *n_samples = (int)ctx->depth.size();
  return GX_OK;
}

int gx_get_depth(gx_ctx* ctx, int sample, gx_depth_hist* out, uint64_t* bases, uint64_t* rsum, uint64_t* rsq, uint64_t* deep_v,
                 uint64_t* deep_bases, size_t cap, size_t* n_deep) {
  if (!ctx || ctx->phase == 1 || ctx->phase == 3 || sample < 0 || (size_t)sample >= ctx->depth.size()) return GX_ERR_ORDER;
  return depth_give(ctx->depth[sample], out, bases, rsum, rsq, deep_v, deep_bases, cap, n_deep);
}

int gx_depth_group(gx_ctx* const* ctxs, int n_ctx, int sample, gx_depth_hist* out, uint64_t* bases, uint64_t* rsum, uint64_t* rsq,
                   uint64_t* deep_v, uint64_t* deep_bases, size_t cap, size_t* n_deep) {
  gx_ctx::DepthResult sum;
  if (int rc = depth_sum(ctxs, n_ctx, sample, sum)) return rc;
  return depth_give(sum, out, bases, rsum, rsq, deep_v, deep_bases, cap, n_deep);
}

int gx_depth_geometry(uint32_t* bound, int* lanes, int* grid, size_t* list_capacity) {
  if (bound) *bound = DEPTH_BOUND;
  if (lanes) *lanes = DEPTH_NW * 64;
  if (grid) *grid = (int)DEPTH_GRID;
  if (list_capacity) *list_capacity = DEPTH_LIST_CAP;
  return GX_OK;
}

int gx_depth_last(gx_ctx* ctx, size_t* list_capacity, int* reruns) {
  if (!ctx) return GX_ERR_ORDER;
  if (list_capacity) *list_capacity = ctx->depthLastCap;
  if (reruns) *reruns = (int)ctx->depthLastReruns;
  return GX_OK;
}

int gx_write_depth_group(gx_ctx* const* ctxs, int n_ctx, FILE* depth, FILE* metrics) {
  if (!ctxs || n_ctx < 1 || !ctxs[0] || (!depth && !metrics)) return GX_ERR_ORDER;
  const size_t nS = ctxs[0]->depth.size();
  if (!nS) return GX_ERR_ORDER;
  std::vector<gx_ctx::DepthResult> sums(nS);
  std::vector<gx_depth_hist> hs(nS);
  for (size_t i = 0; i < nS; i++) {   // (the histograms point into the sums)
    gx_ctx::DepthResult& r = sums[i];
    if (int rc = depth_sum(ctxs, n_ctx, (int)i, r)) return rc;
    (void)depth_give(r, &hs[i], nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
    hs[i].bases = r.bases.data();
    hs[i].rsum = r.rsum.data();
    hs[i].rsq = r.rsq.data();
    hs[i].deep_v = r.deepV.data();
    hs[i].deep_bases = r.deepBases.data();
    hs[i].n_deep = r.deepV.size();
  }
  if (depth)
    if (int rc = gx_format_depth(depth, (int)nS, hs.data())) return rc;
  return metrics ? gx_format_depth_metrics(metrics, (int)nS, hs.data()) : GX_OK;
}

int gx_set_profile(gx_ctx* ctx, const gx_anchor* anchors, size_t n, uint32_t flank, uint32_t bin_size, int keep_matrix) {
  if (!ctx || ctx->nChrom == 0 || ctx->phase != 0 || ctx->sample != 0) return GX_ERR_ORDER;   // idle, and the table is known
  if (n == 0) {   // off
    drop_profile(ctx);
    ctx->profAnchors.clear();
    ctx->profF = ctx->profB = ctx->profNb = 0;
    ctx->profKeep = false;
    return GX_OK;
  }
  const char* why = nullptr;
  if (!anchors) why = "no anchors";
  else if (bin_size == 0) why = "profile bins of 0 bases";
  else if (flank == 0 || flank > PROF_MAX_F) why = "a profile flank outside [1, 2^20]";
  else if (flank % bin_size != 0) why = "the profile's flank is no multiple of its bin size";
  else if (2 * flank / bin_size > PROF_MAX_NB) why = "more than 1024 profile bins";
  else if (n > 0xFFFFFFFFull) why = "more than 2^32 - 1 anchors";
  else if (keep_matrix && (u64)n * (2 * flank / bin_size) > PROF_MAX_CELLS) why = "a profile matrix of more than 2^26 cells";
  for (size_t i = 0; !why && i < n; i++)
    if (anchors[i].strand != 1 && anchors[i].strand != -1) why = "an anchor's strand is neither +1 nor -1";
  if (why) {
    ctx->err = why;
    return GX_ERR_ORDER;
  }
  HIPCHECK(hipSetDevice(ctx->device));
  drop_profile(ctx);
  ctx->profAnchors.assign(anchors, anchors + n);   // (a copy: the caller's array may go away)
  ctx->profF = flank;
  ctx->profB = bin_size;
  ctx->profNb = 2 * flank / bin_size;
  ctx->profKeep = keep_matrix != 0;
  ctx->profDirty = true;
  return prof_layout(ctx);
}

int gx_profile_samples(gx_ctx* ctx, int* n_samples) {
  if (!ctx || !n_samples) return GX_ERR_ORDER;
  *n_samples = (int)ctx->prof.size();
  return GX_OK;
}

int gx_profile_layout(gx_ctx* ctx, size_t* n_anchors, uint32_t* n_bins, uint32_t* flank, uint32_t* bin_size, int* has_matrix) {
  if (!ctx) return GX_ERR_ORDER;
  if (n_anchors) *n_anchors = ctx->profAnchors.size();
  if (n_bins) *n_bins = ctx->profNb;
  if (flank) *flank = ctx->profF;
  if (bin_size) *bin_size = ctx->profB;
  if (has_matrix) *has_matrix = ctx->profKeep ? 1 : 0;
  return GX_OK;
}

int gx_get_profile(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, int64_t* agg120, int64_t* cell120, size_t first_anchor,
                   size_t n_rows) {
  if (!ctx || ctx->phase == 1 || ctx->phase == 3 || sample < 0 || (size_t)sample >= ctx->prof.size()) return GX_ERR_ORDER;
  const gx_ctx::ProfSample& p = ctx->prof[sample];
  const size_t nA = ctx->profAnchors.size(), nb = ctx->profNb;
  if (cell120 && (!p.cells.p || first_anchor > nA || n_rows > nA - first_anchor)) return GX_ERR_ORDER;
  if (rep) *rep = p.rep;
  if (is_ctrl) *is_ctrl = p.ctrl ? 1 : 0;
  if (!agg120 && !(cell120 && n_rows)) return GX_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  if (agg120) HIPCHECK(hipMemcpyAsync(agg120, p.agg.p, nb * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (cell120 && n_rows)
    HIPCHECK(hipMemcpyAsync(cell120, p.cells.as<int64_t>() + first_anchor * nb, n_rows * nb * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  return GX_OK;
}

int gx_write_profile_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, const char* const* sample_names, size_t n_anchors_counted,
                           FILE* out) {
  if (!ctxs || n_ctx < 1 || !out || n_samples < 0 || (n_samples && !sample_names)) return GX_ERR_ORDER;
  uint32_t nb = 0, F = 0, B = 0;
  if (int rc = gx_profile_layout(ctxs[0], nullptr, &nb, &F, &B, nullptr)) return rc;
  std::vector<int64_t> agg((size_t)n_samples * nb, 0), one(nb);
  for (int g = 0; g < n_ctx; g++)
    for (int smp = 0; smp < n_samples; smp++) {
      if (int rc = gx_get_profile(ctxs[g], smp, nullptr, nullptr, one.data(), nullptr, 0, 0)) return rc;
      for (uint32_t j = 0; j < nb; j++) agg[(size_t)smp * nb + j] += one[j];
    }
  std::vector<const int64_t*> rows((size_t)n_samples);
  for (int smp = 0; smp < n_samples; smp++) rows[smp] = agg.data() + (size_t)smp * nb;
  return gx_format_profile(out, n_samples, sample_names, rows.data(), n_anchors_counted, nb, F, B);
}

int gx_write_profile_rows_group(gx_ctx* const* ctxs, int n_ctx, int sample, const char* const* names, const gx_region* regions,
                                const char* const* row_names, const gx_anchor* anchors, FILE* out) {
  if (!ctxs || n_ctx < 1 || !out) return GX_ERR_ORDER;
  size_t nA = 0;
  uint32_t nb = 0, B = 0;
  if (int rc = gx_profile_layout(ctxs[0], &nA, &nb, nullptr, &B, nullptr)) return rc;
  if (!nb) return GX_ERR_ORDER;
  const size_t chunk = std::max<size_t>(1, (1u << 20) / nb);   // (8 MiB of cells at a time)
  std::vector<int64_t> sum, one;
  for (size_t first = 0; first < nA; first += chunk) {
    const size_t rows = std::min(chunk, nA - first);
    sum.assign(rows * nb, 0);
    one.resize(rows * nb);
    for (int g = 0; g < n_ctx; g++) {
      if (int rc = gx_get_profile(ctxs[g], sample, nullptr, nullptr, nullptr, one.data(), first, rows)) return rc;
      for (size_t k = 0; k < rows * nb; k++) sum[k] += one[k];
    }
    if (int rc = gx_format_profile_rows(out, names, regions, row_names, anchors, first, rows, nb, B, sum.data())) return rc;
  }
  return GX_OK;
}

int gx_coverage_gram(gx_ctx* ctx, int* n_samples, uint64_t* n_bins, uint64_t* n_zero, gx_u128* sum, gx_u128* gram, int cap) {
  BinRows b;
  if (int rc = stat_cov_rows(ctx, "the correlation", b)) return rc;
  if (int rc = stat_cap(ctx, "gx_coverage_gram", sum || gram, cap, b.rows.size())) return rc;
  if ((u128)ctx->covW * (u128)b.G > ((u128)1 << 64))
    return refuse(ctx, "bin size times genome length above 2^64: the correlation's sums could overflow");
  HIPCHECK(hipSetDevice(ctx->device));
  u64 nz = 0;
  std::vector<gx_u128> s1, g1;
  if (int rc = gram_pass(ctx, b.rows, b.n, 0, &nz, s1, g1)) return rc;
  if (n_samples) *n_samples = (int)b.rows.size();
  if (n_bins) *n_bins = b.n;
  if (n_zero) *n_zero = nz;
  stat_give_sums(s1, g1, sum, gram, (size_t)cap);
  return GX_OK;
}

int gx_gram_u64(gx_ctx* ctx, const uint64_t* rows, int n_rows, size_t n, unsigned grid, uint64_t* n_zero, gx_u128* sum, gx_u128* gram) {
  if (int rc = stat_u64_domain(ctx, "gx_gram_u64", rows, n_rows, n, grid, true)) return rc;
  std::vector<const void*> dev;
  if (int rc = stat_stage_rows(ctx, rows, n_rows, n, dev)) return rc;
  u64 nz = 0;
  std::vector<gx_u128> s1, g1;
  if (int rc = gram_pass(ctx, dev, n, grid, &nz, s1, g1)) return rc;
  if (n_zero) *n_zero = nz;
  stat_give_sums(s1, g1, sum, gram, (size_t)n_rows);
  return GX_OK;
}

int gx_gram_geometry(int* tile, int* lanes, int* grid) {
  if (tile) *tile = GRAM_T;
  if (lanes) *lanes = GRAM_NW * 64;
  if (grid) *grid = (int)GRAM_GRID;
  return GX_OK;
}

int gx_coverage_gram_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, uint64_t* n_bins, uint64_t* n_zero, gx_u128* sum, gx_u128* gram) {
  if (!ctxs || n_ctx < 1 || n_samples < 1 || n_samples > (int)GRAM_MAX_S || !sum || !gram) return GX_ERR_ORDER;
  Sums128 total((size_t)n_samples);
  uint64_t n = 0, nz = 0;
  for (int g = 0; g < n_ctx; g++) {
    int s = 0;
    uint64_t n1 = 0, nz1 = 0;
    if (int rc = gx_coverage_gram(ctxs[g], &s, &n1, &nz1, sum, gram, n_samples)) return rc;
    if (s != n_samples) return GX_ERR_ORDER;
    n += n1;
    nz += nz1;
    total.add(sum, gram);
  }
  total.give(sum, gram);
  if (n_bins) *n_bins = n;
  if (n_zero) *n_zero = nz;
  return GX_OK;
}

int gx_write_correlation_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, const char* const* sample_names, int skip_zeros, FILE* out) {
  if (!out || !sample_names || n_samples < 1 || n_samples > (int)GRAM_MAX_S) return GX_ERR_ORDER;
  std::vector<gx_u128> s1((size_t)n_samples), g1((size_t)n_samples * n_samples);
  uint64_t n = 0, nz = 0;
  if (int rc = gx_coverage_gram_group(ctxs, n_ctx, n_samples, &n, &nz, s1.data(), g1.data())) return rc;
  return gx_format_correlation(out, n_samples, sample_names, n, nz, s1.data(), g1.data(), skip_zeros);
}

int gx_coverage_fingerprint(gx_ctx* ctx, int* n_samples, uint64_t* n_bins, uint64_t* count, uint64_t* sum, int cap) {
  BinRows b;
  if (int rc = stat_cov_rows(ctx, "the fingerprint", b)) return rc;
  if (int rc = stat_cap(ctx, "gx_coverage_fingerprint", count || sum, cap, b.rows.size())) return rc;
  if (b.G >= ((u64)1 << 33)) return refuse(ctx, "a genome of 2^33 bases or more: the fingerprint's sums could overflow");
  HIPCHECK(hipSetDevice(ctx->device));
  std::vector<uint64_t> c1, s1;
  if (int rc = fp_pass(ctx, b.rows, b.n, 0, c1, s1)) return rc;
  if (n_samples) *n_samples = (int)b.rows.size();
  if (n_bins) *n_bins = b.n;
  if (count) std::copy(c1.begin(), c1.end(), count);
  if (sum) std::copy(s1.begin(), s1.end(), sum);
  return GX_OK;
}

int gx_fp_u64(gx_ctx* ctx, const uint64_t* rows, int n_rows, size_t n, unsigned grid, uint64_t* count, uint64_t* sum) {
  if (int rc = stat_u64_domain(ctx, "gx_fp_u64", rows, n_rows, n, grid, false)) return rc;
  // every row is added in 128 bits: a total of 2^64 or more is refused before anything reaches the device
  for (int r = 0; r < n_rows; r++) {
    u128 t = 0;
    for (size_t k = 0; k < n; k++) t += rows[(size_t)r * n + k];
    if (t >> 64) return refuse(ctx, "gx_fp_u64: a row's total of 2^64 or more");
  }
  std::vector<const void*> dev;
  if (int rc = stat_stage_rows(ctx, rows, n_rows, n, dev)) return rc;
  std::vector<uint64_t> c1, s1;
  if (int rc = fp_pass(ctx, dev, n, grid, c1, s1)) return rc;
  if (count) std::copy(c1.begin(), c1.end(), count);
  if (sum) std::copy(s1.begin(), s1.end(), sum);
  return GX_OK;
}

int gx_fp_geometry(int* n_classes, int* sub_log, int* lanes, int* grid) {
  if (n_classes) *n_classes = FP_NC;
  if (sub_log) *sub_log = GX_FP_SUB_LOG;
  if (lanes) *lanes = FP_NW * 64;
  if (grid) *grid = (int)FP_GRID;
  return GX_OK;
}

int gx_coverage_fingerprint_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, uint64_t* n_bins, uint64_t* count, uint64_t* sum) {
  if (!ctxs || n_ctx < 1 || n_samples < 1 || n_samples > (int)FP_MAX_S || !count || !sum) return GX_ERR_ORDER;
  const size_t N = (size_t)n_samples * FP_NC;
  std::vector<uint64_t> ct(N, 0), st(N, 0);
  uint64_t n = 0;
  for (int g = 0; g < n_ctx; g++) {
    int s = 0;
    uint64_t n1 = 0;
    if (int rc = gx_coverage_fingerprint(ctxs[g], &s, &n1, count, sum, n_samples)) return rc;
    if (s != n_samples) return GX_ERR_ORDER;
    n += n1;
    for (size_t k = 0; k < N; k++) {
      ct[k] += count[k];
      st[k] += sum[k];
    }
  }
  std::copy(ct.begin(), ct.end(), count);
  std::copy(st.begin(), st.end(), sum);
  if (n_bins) *n_bins = n;
  return GX_OK;
}

int gx_write_fingerprint_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, const char* const* sample_names, const int* ctrl_of, FILE* curve,
                               FILE* metrics) {
  if (!curve || !sample_names || n_samples < 1 || n_samples > (int)FP_MAX_S) return GX_ERR_ORDER;
  std::vector<uint64_t> c1((size_t)n_samples * FP_NC), s1((size_t)n_samples * FP_NC);
  if (int rc = gx_coverage_fingerprint_group(ctxs, n_ctx, n_samples, nullptr, c1.data(), s1.data())) return rc;
  if (int rc = gx_format_fingerprint(curve, n_samples, sample_names, c1.data(), s1.data())) return rc;
  return metrics ? gx_format_fingerprint_metrics(metrics, n_samples, sample_names, c1.data(), s1.data(), ctrl_of) : GX_OK;
}

int gx_coverage_distinct(gx_ctx* ctx, int sample, uint64_t* value, uint64_t* count, size_t cap, size_t* n_distinct) {
  BinRows b;
  if (int rc = rank_cov_rows(ctx, b)) return rc;
  if (sample < 0 || (size_t)sample >= b.rows.size() || (cap && (!value || !count))) return GX_ERR_ORDER;
  std::vector<uint64_t> v, c;
  if (int rc = rank_distinct_pass(ctx, b.rows[sample], b.n, 0, v, c)) return rc;
  return rank_give_table(ctx, "gx_coverage_distinct", v, c, value, count, cap, n_distinct);
}

int gx_distinct_u64(gx_ctx* ctx, const uint64_t* row, size_t n, unsigned grid, uint64_t* value, uint64_t* count, size_t cap,
                    size_t* n_distinct) {
  if (int rc = stat_u64_domain(ctx, "gx_distinct_u64", row, 1, n, grid, true)) return rc;
  if (cap && (!value || !count)) return GX_ERR_ORDER;
  std::vector<const void*> dev;
  if (int rc = stat_stage_rows(ctx, row, 1, n, dev)) return rc;
  std::vector<uint64_t> v, c;
  if (int rc = rank_distinct_pass(ctx, dev[0], n, grid, v, c)) return rc;
  return rank_give_table(ctx, "gx_distinct_u64", v, c, value, count, cap, n_distinct);
}

int gx_rank_u64(gx_ctx* ctx, const uint64_t* rows, int n_rows, size_t n, unsigned grid, int skip_zeros, uint64_t* rank2, uint64_t* n_zero) {
  if (int rc = stat_u64_domain(ctx, "gx_rank_u64", rows, n_rows, n, grid, true)) return rc;
  std::vector<RankGroup> one(1, RankGroup{ctx, {}, n});
  if (int rc = stat_stage_rows(ctx, rows, n_rows, n, one[0].rows)) return rc;
  RankTables t;
  if (int rc = rank_make_tables(one, grid, skip_zeros != 0, "gx_rank_u64: the rows' tables do not make rank tables", t)) return rc;
  std::vector<const void*> out;
  u64 nz = 0;
  if (int rc = rank_rows_pass(ctx, one[0].rows, n, grid, skip_zeros != 0, t.lut.data(), out, &nz)) return rc;
  if (n_zero) *n_zero = nz;
  if (rank2 && n) {
    for (int i = 0; i < n_rows; i++)
      HIPCHECK(hipMemcpyAsync(rank2 + (size_t)i * n, out[i], n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
  }
  return GX_OK;
}

int gx_rank_geometry(int* lanes, int* grid, int* cache_entries, size_t* first_capacity, size_t* load_limit) {
  if (lanes) *lanes = RK_NW * 64;
  if (grid) *grid = (int)RK_GRID;
  if (cache_entries) *cache_entries = (int)RK_CACHE;
  if (first_capacity) *first_capacity = (size_t)1 << RK_CAP_LOG;
  if (load_limit) *load_limit = ((size_t)1 << RK_CAP_LOG) / RK_LOAD_DIV;
  return GX_OK;
}

int gx_rank_last(gx_ctx* ctx, size_t* capacity, int* n_grown) {
  if (!ctx) return GX_ERR_ORDER;
  if (capacity) *capacity = ctx->rankLastCapLog ? (size_t)1 << ctx->rankLastCapLog : 0;
  if (n_grown) *n_grown = (int)ctx->rankLastGrown;
  return GX_OK;
}

int gx_coverage_rank_gram(gx_ctx* ctx, const gx_rank_lut* tables, int skip_zeros, int* n_samples, uint64_t* n_bins, uint64_t* n_zero,
                          gx_u128* sum, gx_u128* gram, int cap) {
  BinRows b;
  if (int rc = rank_cov_rows(ctx, b)) return rc;
  const size_t S = b.rows.size();
  if (!tables || !rank_lut_ok(tables, S))
    return refuse(ctx, "gx_coverage_rank_gram: a table is not ascending, holds the value 2^64 - 1, or a rank is outside [1, 2^42)");
  if (int rc = stat_cap(ctx, "gx_coverage_rank_gram", sum || gram, cap, S)) return rc;
  std::vector<const void*> ranks;
  u64 nz = 0, nzGram = 0;
  if (int rc = rank_rows_pass(ctx, b.rows, b.n, 0, skip_zeros != 0, tables, ranks, &nz)) return rc;
  std::vector<gx_u128> s1, g1;
  if (int rc = gram_pass(ctx, ranks, b.n, 0, &nzGram, s1, g1)) return rc;
  if (skip_zeros && nzGram != nz) {   // (a rank is at least 1: the rows that are 0 everywhere are the bins left out)
    ctx->err = "gx_coverage_rank_gram: the rank rows' zero bins are not the bins left out";
    return GX_ERR_DEVICE;
  }
  if (n_samples) *n_samples = (int)S;
  if (n_bins) *n_bins = b.n;
  if (n_zero) *n_zero = nz;
  stat_give_sums(s1, g1, sum, gram, (size_t)cap);
  return GX_OK;
}

int gx_coverage_spearman_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, int skip_zeros, uint64_t* n_ranked, gx_u128* sum, gx_u128* gram,
                               uint64_t* n_distinct) {
  if (!ctxs || n_ctx < 1 || n_samples < 1 || n_samples > (int)RK_MAX_S || !sum || !gram) return GX_ERR_ORDER;
  const size_t S = (size_t)n_samples;
  // 1. every context's rows, then the rank tables over all contexts (with skip_zeros without the all-zero bins)
  std::vector<RankGroup> groups;
  for (int g = 0; g < n_ctx; g++) {
    BinRows b;
    if (int rc = rank_cov_rows(ctxs[g], b)) return rc;
    if (b.rows.size() != S) return refuse(ctxs[g], "gx_coverage_spearman_group: a context has another number of samples");
    groups.push_back(RankGroup{ctxs[g], std::move(b.rows), b.n});
  }
  RankTables t;
  if (int rc = rank_make_tables(groups, 0, skip_zeros != 0, "the contexts' tables do not make rank tables (more than 2^41 bins?)", t)) return rc;
  // 2. every context's rank rows and their sums, added with carries
  Sums128 total(S);
  uint64_t nzSeen = 0;
  for (int g = 0; g < n_ctx; g++) {
    uint64_t nz1 = 0;
    if (int rc = gx_coverage_rank_gram(ctxs[g], t.lut.data(), skip_zeros, nullptr, nullptr, &nz1, sum, gram, n_samples)) return rc;
    nzSeen += nz1;
    total.add(sum, gram);
  }
  if (skip_zeros && nzSeen != t.nZero) {
    for (int g = 0; g < n_ctx; g++) ctxs[g]->err = "gx_coverage_spearman_group: the bins left out are not the all-zero bins counted";
    return GX_ERR_DEVICE;
  }
  total.give(sum, gram);
  if (n_ranked) *n_ranked = t.nRanked;
  if (n_distinct) std::copy(t.nDistinct.begin(), t.nDistinct.end(), n_distinct);
  return GX_OK;
}

int gx_write_spearman_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, const char* const* sample_names, int skip_zeros, FILE* out) {
  if (!out || !sample_names || n_samples < 1 || n_samples > (int)RK_MAX_S) return GX_ERR_ORDER;
  std::vector<gx_u128> s1((size_t)n_samples), g1((size_t)n_samples * n_samples);
  uint64_t N = 0;
  if (int rc = gx_coverage_spearman_group(ctxs, n_ctx, n_samples, skip_zeros, &N, s1.data(), g1.data(), nullptr)) return rc;
  return gx_format_correlation(out, n_samples, sample_names, N, 0, s1.data(), g1.data(), 0);
}

int gx_peak_signal(gx_ctx* ctx, int* n_samples) {
  if (!ctx || !ctx->countOn || !ctx->peaksReady || ctx->phase != 0) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  ctx->psigReady = false;
  if (int rc = peak_signal_kept(ctx)) return rc;
  if (n_samples) *n_samples = (int)ctx->kept.size();
  return GX_OK;
}

int gx_get_peak_signal(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, int64_t* area120, int64_t* max120, uint32_t* summit, uint32_t* covered,
                       int64_t* at_summit120, size_t cap) {
  if (!ctx || !ctx->psigReady || sample < 0 || (size_t)sample >= ctx->kept.size()) return GX_ERR_ORDER;
  if (rep) *rep = ctx->kept[sample].rep;
  if (is_ctrl) *is_ctrl = ctx->kept[sample].ctrl ? 1 : 0;
  psig_give(static_cast<const PsigRec*>(ctx->psigHost.p) + (size_t)sample * ctx->psigPk, ctx->psigPk, cap, area120, max120, summit, covered, at_summit120);
  return GX_OK;
}

int gx_peak_signal_events(gx_ctx* ctx, const gx_event* ev, size_t n, const gx_region* peaks, size_t n_peaks, const uint32_t* summit_off, unsigned grid,
                          int64_t* area120, int64_t* max120, uint32_t* summit, uint32_t* covered, int64_t* at_summit120) {
  if (!ctx || ctx->nChrom == 0 || (n && !ev) || (n_peaks && !peaks)) return GX_ERR_ORDER;
  if (int rc = guard_closed(ctx, "gx_peak_signal_events")) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  if (int rc = peak_signal_events(ctx, ev, n, peaks, n_peaks, summit_off, grid)) return rc;
  psig_give(static_cast<const PsigRec*>(ctx->psigEvHost.p), n_peaks, n_peaks, area120, max120, summit, covered, at_summit120);
  return GX_OK;
}

int gx_peak_signal_geometry(int* lanes, int* grid, uint32_t* step_bases, uint32_t* slot_pad, uint64_t* max_events) {
  if (lanes) *lanes = PSIG_NT;
  if (grid) *grid = (int)PSIG_GRID;
  if (step_bases) *step_bases = PSIG_STEP;
  if (slot_pad) *slot_pad = PSIG_PAD;
  if (max_events) *max_events = PSIG_MAX_EVENTS - 1;
  return GX_OK;
}

int gx_write_peak_signal_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, FILE* out) {
  if (!ctxs || n_ctx < 1 || !names || !out) return GX_ERR_ORDER;
  int nS = 0;
  if (int rc = pass_on_all(ctxs, n_ctx, gx_peak_signal, &nS)) return rc;
  gx_peak_merge::Merged m;
  if (int rc = gx_peak_merge::merged_peaks(ctxs, n_ctx, m)) return rc;
  // every sample's five columns: the contexts' one after the other, then in the merged order
  std::vector<std::vector<int64_t>> area((size_t)nS), mx((size_t)nS), at((size_t)nS);
  std::vector<std::vector<uint32_t>> sm((size_t)nS), cov((size_t)nS);
  std::vector<int> rep((size_t)nS), ctrl((size_t)nS);
  std::vector<const int64_t*> pa, pm, pt;
  std::vector<const uint32_t*> ps, pc;
  for (int i = 0; i < nS; i++) {
    area[i].resize(m.size()); mx[i].resize(m.size()); at[i].resize(m.size()); sm[i].resize(m.size()); cov[i].resize(m.size());
    for (int g = 0; g < n_ctx; g++) {
      const size_t at0 = m.first[g];
      if (int rc = gx_get_peak_signal(ctxs[g], i, &rep[i], &ctrl[i], area[i].data() + at0, mx[i].data() + at0, sm[i].data() + at0, cov[i].data() + at0,
                                      at[i].data() + at0, m.first[g + 1] - at0))
        return rc;
    }
    area[i] = permuted(m, area[i]); mx[i] = permuted(m, mx[i]); at[i] = permuted(m, at[i]); sm[i] = permuted(m, sm[i]); cov[i] = permuted(m, cov[i]);
    pa.push_back(area[i].data()); pm.push_back(mx[i].data()); pt.push_back(at[i].data()); ps.push_back(sm[i].data()); pc.push_back(cov[i].data());
  }
  return gx_format_peak_signal(out, names, m.regions.data(), m.size(), nS, rep.data(), ctrl.data(), pa.data(), pm.data(), ps.data(), pc.data(), pt.data());
}

int gx_write_peak_signal(gx_ctx* ctx, const char* const* names, FILE* out) { return gx_write_peak_signal_group(&ctx, 1, names, out); }

int gx_peak_summits(gx_ctx* ctx, int prominence_pct, int height_pct, size_t* n) {
  if (!ctx || !ctx->countOn || !ctx->peaksReady || ctx->phase != 0) return GX_ERR_ORDER;
  if (prominence_pct < 0 || prominence_pct > 100 || height_pct < 0 || height_pct > 100) return refuse(ctx, "gx_peak_summits: a percentage outside 0..100");
  HIPCHECK(hipSetDevice(ctx->device));
  ctx->sumReady = false;
  if (int rc = peak_summits_kept(ctx, (u32)prominence_pct, (u32)height_pct)) return rc;
  if (n) *n = ctx->sumRes.size();
  return GX_OK;
}

int gx_get_peak_summits(gx_ctx* ctx, gx_summit* out, size_t cap) {
  if (!ctx || !ctx->sumReady || (cap && !out)) return GX_ERR_ORDER;
  if (const size_t m = std::min(cap, ctx->sumRes.size())) memcpy(out, ctx->sumRes.data(), m * sizeof(gx_summit));
  return GX_OK;
}

int gx_peak_summits_events(gx_ctx* ctx, const gx_event* ev, size_t n, const gx_region* peaks, size_t n_peaks, int prominence_pct, int height_pct,
                           unsigned grid, unsigned run_cap, size_t list_cap, gx_summit* out, size_t cap, size_t* n_out) {
  if (!ctx || ctx->nChrom == 0 || (n && !ev) || (n_peaks && !peaks) || (cap && !out)) return GX_ERR_ORDER;
  if (int rc = guard_closed(ctx, "gx_peak_summits_events")) return rc;
  if (prominence_pct < 0 || height_pct < 0) return refuse(ctx, "gx_peak_summits_events: a negative percentage");
  HIPCHECK(hipSetDevice(ctx->device));
  std::vector<gx_summit> res;
  if (int rc = peak_summits_events(ctx, ev, n, peaks, n_peaks, (u32)prominence_pct, (u32)height_pct, grid, run_cap, list_cap, res)) return rc;
  if (const size_t m = std::min(cap, res.size())) memcpy(out, res.data(), m * sizeof(gx_summit));
  if (n_out) *n_out = res.size();
  return GX_OK;
}

int gx_peak_summits_last(gx_ctx* ctx, unsigned* reruns, unsigned* big_peaks) {
  if (!ctx) return GX_ERR_ORDER;
  if (reruns) *reruns = ctx->sumLastReruns;
  if (big_peaks) *big_peaks = ctx->sumLastBig;
  return GX_OK;
}

int gx_peak_summits_geometry(int* lanes, int* grid, uint32_t* step_bases, uint32_t* run_cap, uint64_t* list_min, uint32_t* list_per_peak,
                             uint64_t* max_events) {
  if (lanes) *lanes = SUM_NT;
  if (grid) *grid = (int)SUM_GRID;
  if (step_bases) *step_bases = PSIG_STEP;
  if (run_cap) *run_cap = SUM_RUN_CAP;
  if (list_min) *list_min = SUM_LIST_MIN;
  if (list_per_peak) *list_per_peak = 2;
  if (max_events) *max_events = PSIG_MAX_EVENTS - 1;
  return GX_OK;
}

int gx_write_summits_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, int prominence_pct, int height_pct, FILE* out) {
  if (!ctxs || n_ctx < 1 || !names || !out) return GX_ERR_ORDER;
  int none = 0;
  if (int rc = pass_on_all(ctxs, n_ctx, [&](gx_ctx* c, int*) { return gx_peak_summits(c, prominence_pct, height_pct, nullptr); }, &none)) return rc;
  gx_peak_merge::Merged m;
  if (int rc = gx_peak_merge::merged_peaks(ctxs, n_ctx, m)) return rc;
  std::vector<std::vector<gx_summit>> own;
  for (int g = 0; g < n_ctx; g++) own.push_back(ctxs[g]->sumRes);
  const std::vector<gx_summit> sm = renumbered(m, own, &gx_summit::peak, gx_peak_merge::summit_less);
  return gx_format_summits(out, names, m.regions.data(), m.size(), sm.data(), sm.size());
}

int gx_write_summits(gx_ctx* ctx, const char* const* names, int prominence_pct, int height_pct, FILE* out) {
  return gx_write_summits_group(&ctx, 1, names, prominence_pct, height_pct, out);
}

int gx_complexity(gx_ctx* ctx, int* n_samples) {
  if (!ctx) return GX_ERR_ORDER;
  if (int rc = guard_kept(ctx, "gx_complexity", true)) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  ctx->cpxReady = false;
  if (int rc = complexity_kept(ctx)) return rc;
  if (n_samples) *n_samples = (int)ctx->cpx.size();
  return GX_OK;
}

int gx_get_complexity(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, uint64_t* n_obs, uint64_t* n_distinct, uint64_t* mult, uint64_t* keys,
                      size_t cap, size_t* n_classes) {
  if (!ctx || !ctx->cpxReady || sample < 0 || (size_t)sample >= ctx->cpx.size()) return GX_ERR_ORDER;
  return cpx_give(ctx->cpx[sample], rep, is_ctrl, n_obs, n_distinct, mult, keys, cap, n_classes);
}

int gx_complexity_events(gx_ctx* ctx, const gx_event* ev, size_t n, unsigned grid, int cap_log, uint64_t* n_obs, uint64_t* n_distinct,
                         uint64_t* mult, uint64_t* keys, size_t cap, size_t* n_classes) {
  if (!ctx || ctx->nChrom == 0 || (n && !ev) || cap_log < 0 || (cap && (!mult || !keys))) return GX_ERR_ORDER;
  if (int rc = guard_closed(ctx, "gx_complexity_events")) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  gx_ctx::CpxResult r;
  if (int rc = complexity_events(ctx, ev, n, grid, cap_log, r)) return rc;
  return cpx_give(r, nullptr, nullptr, n_obs, n_distinct, mult, keys, cap, n_classes);
}

int gx_complexity_geometry(int* lanes, int* grid, uint32_t* lds_bound, uint64_t n, size_t* least_capacity) {
  if (lanes) *lanes = CPX_NT;
  if (grid) *grid = (int)CPX_GRID;
  if (lds_bound) *lds_bound = CPX_BOUND;
  if (least_capacity) *least_capacity = n >> 31 ? 0 : (size_t)1 << cpx_least_cap_log(n);
  return GX_OK;
}

int gx_complexity_last(gx_ctx* ctx, size_t* capacity) {
  if (!ctx) return GX_ERR_ORDER;
  if (capacity) *capacity = ctx->cpxLastCapLog ? (size_t)1 << ctx->cpxLastCapLog : 0;
  return GX_OK;
}

int gx_complexity_group(gx_ctx* const* ctxs, int n_ctx, int sample, int* rep, int* is_ctrl, uint64_t* n_obs, uint64_t* n_distinct, uint64_t* mult,
                        uint64_t* keys, size_t cap, size_t* n_classes) {
  gx_ctx::CpxResult sum;
  if (int rc = cpx_sum(ctxs, n_ctx, sample, sum)) return rc;
  return cpx_give(sum, rep, is_ctrl, n_obs, n_distinct, mult, keys, cap, n_classes);
}

int gx_write_complexity_group(gx_ctx* const* ctxs, int n_ctx, FILE* metrics, FILE* hist) {
  if (!ctxs || n_ctx < 1 || !metrics) return GX_ERR_ORDER;
  int nS = 0;
  if (int rc = pass_on_all(ctxs, n_ctx, gx_complexity, &nS)) return rc;
  std::vector<gx_ctx::CpxResult> sums((size_t)nS);   // (each sample summed once; the writers read the sums in place)
  std::vector<int> rep, ctrl;
  std::vector<uint64_t> N, D;
  std::vector<const uint64_t*> pm, pk;
  std::vector<size_t> np;
  for (int i = 0; i < nS; i++) {
    const gx_ctx::CpxResult& r = sums[i];
    if (int rc = cpx_sum(ctxs, n_ctx, i, sums[i])) return rc;
    rep.push_back(r.rep); ctrl.push_back(r.ctrl); N.push_back(r.N); D.push_back(r.D);
    pm.push_back(r.mult.data()); pk.push_back(r.keys.data()); np.push_back(r.mult.size());
  }
  if (int rc = gx_format_complexity(metrics, nS, rep.data(), ctrl.data(), N.data(), D.data(), pm.data(), pk.data(), np.data())) return rc;
  return hist ? gx_format_complexity_hist(hist, nS, rep.data(), ctrl.data(), pm.data(), pk.data(), np.data()) : GX_OK;
}

int gx_interval_stats(gx_ctx* ctx, int* n_samples) {
  if (!ctx) return GX_ERR_ORDER;
  if (int rc = guard_kept(ctx, "gx_interval_stats", true)) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  ctx->ivsReady = false;
  if (int rc = ivstat_kept(ctx)) return rc;
  if (n_samples) *n_samples = (int)ctx->ivs.size();
  return GX_OK;
}

int gx_get_interval_lengths(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, uint64_t* length, uint64_t* n, uint64_t* w120, size_t cap,
                            size_t* n_classes, uint64_t* n_inverted, uint64_t* w120_inverted) {
  if (!ctx || !ctx->ivsReady || sample < 0 || (size_t)sample >= ctx->ivs.size()) return GX_ERR_ORDER;
  return ivs_give(ctx->ivs[sample], rep, is_ctrl, length, n, w120, cap, n_classes, n_inverted, w120_inverted, nullptr, nullptr, nullptr, 0);
}

int gx_get_chrom_stats(gx_ctx* ctx, int sample, uint64_t* cn, uint64_t* cw120, uint64_t* cbases120, size_t cap) {
  if (!ctx || !ctx->ivsReady || sample < 0 || (size_t)sample >= ctx->ivs.size()) return GX_ERR_ORDER;
  return ivs_give(ctx->ivs[sample], nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, cn, cw120, cbases120, cap);
}

int gx_interval_stats_events(gx_ctx* ctx, const gx_event* ev, size_t n, unsigned grid, size_t list_cap, uint64_t* length, uint64_t* n_iv,
                             uint64_t* w120, size_t cap, size_t* n_classes, uint64_t* n_inverted, uint64_t* w120_inverted, uint64_t* cn,
                             uint64_t* cw120, uint64_t* cbases120, size_t chrom_cap) {
  if (!ctx || ctx->nChrom == 0 || (n && !ev) || (cap && (!length || !n_iv || !w120)) || (chrom_cap && (!cn || !cw120 || !cbases120))) return GX_ERR_ORDER;
  if (int rc = guard_closed(ctx, "gx_interval_stats_events")) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  gx_ctx::IvsResult r;
  if (int rc = ivstat_events(ctx, ev, n, grid, list_cap, r)) return rc;
  return ivs_give(r, nullptr, nullptr, length, n_iv, w120, cap, n_classes, n_inverted, w120_inverted, cn, cw120, cbases120, chrom_cap);
}

int gx_interval_stats_geometry(int* lanes, int* grid, uint32_t* lds_bound, uint32_t* chrom_window, size_t* list_capacity) {
  static_assert(IVS_BOUND == GX_IVS_BOUND, "the header's bound is the kernel's");
  if (lanes) *lanes = CNT_NT;
  if (grid) *grid = (int)IVS_GRID;
  if (lds_bound) *lds_bound = IVS_BOUND;
  if (chrom_window) *chrom_window = IVS_CHROM_WINDOW;
  if (list_capacity) *list_capacity = IVS_LIST_CAP;
  return GX_OK;
}

int gx_interval_stats_last(gx_ctx* ctx, size_t* list_capacity, int* reruns) {
  if (!ctx) return GX_ERR_ORDER;
  if (list_capacity) *list_capacity = ctx->ivsLastCap;
  if (reruns) *reruns = (int)ctx->ivsLastReruns;
  return GX_OK;
}

int gx_interval_stats_group(gx_ctx* const* ctxs, int n_ctx, int sample, int* rep, int* is_ctrl, uint64_t* length, uint64_t* n, uint64_t* w120,
                            size_t cap, size_t* n_classes, uint64_t* n_inverted, uint64_t* w120_inverted, uint64_t* cn, uint64_t* cw120,
                            uint64_t* cbases120, size_t chrom_cap) {
  gx_ctx::IvsResult sum;
  if (int rc = ivs_sum(ctxs, n_ctx, sample, sum)) return rc;
  return ivs_give(sum, rep, is_ctrl, length, n, w120, cap, n_classes, n_inverted, w120_inverted, cn, cw120, cbases120, chrom_cap);
}

int gx_write_interval_stats_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, int n_chrom, int cut_sites, const uint64_t* cuts,
                                  int n_cuts, FILE* lengths, FILE* metrics, FILE* chroms) {
  if (!ctxs || n_ctx < 1 || !ctxs[0] || (!lengths && !metrics && !chroms) || (chroms && (!names || n_chrom != (int)ctxs[0]->nChrom))) return GX_ERR_ORDER;
  int nS = 0;
  if (int rc = pass_on_all(ctxs, n_ctx, gx_interval_stats, &nS)) return rc;
  const size_t nC = ctxs[0]->nChrom;
  std::vector<gx_ctx::IvsResult> sums((size_t)nS);   // (each sample summed once; the writers read the sums in place)
  std::vector<int> rep, ctrl;
  std::vector<uint64_t> nInv, wInv;
  std::vector<const uint64_t*> pl, pn, pw, pcn, pcw, pcb;
  std::vector<size_t> np;
  for (int i = 0; i < nS; i++) {
    const gx_ctx::IvsResult& r = sums[i];
    if (int rc = ivs_sum(ctxs, n_ctx, i, sums[i])) return rc;
    rep.push_back(r.rep); ctrl.push_back(r.ctrl); nInv.push_back(r.nInv); wInv.push_back(r.wInv);
    pl.push_back(r.len.data()); pn.push_back(r.n.data()); pw.push_back(r.w.data()); np.push_back(r.len.size());
    pcn.push_back(r.cn.data()); pcw.push_back(r.cw.data()); pcb.push_back(r.cb.data());
  }
  if (lengths)
    if (int rc = gx_format_lengths(lengths, nS, rep.data(), ctrl.data(), pl.data(), pn.data(), pw.data(), np.data(), nInv.data(), wInv.data(), cut_sites)) return rc;
  if (metrics)
    if (int rc = gx_format_lengths_metrics(metrics, nS, rep.data(), ctrl.data(), pl.data(), pn.data(), pw.data(), np.data(), cuts, n_cuts)) return rc;
  if (chroms) {
    std::vector<uint32_t> lens(nC);
    for (size_t c = 0; c < nC; c++) lens[c] = ctxs[0]->hChrom[c].len;
    if (int rc = gx_format_chrom_stats(chroms, names, lens.data(), (int)nC, nS, rep.data(), ctrl.data(), pcn.data(), pcw.data(), pcb.data())) return rc;
  }
  return GX_OK;
}

int gx_set_xcor(gx_ctx* ctx, int lo, int hi) {
  if (!ctx || ctx->nChrom == 0 || ctx->phase != 0 || ctx->sample != 0) return GX_ERR_ORDER;   // idle, and the table is known
  HIPCHECK(hipSetDevice(ctx->device));
  drop_xcor(ctx);
  if (hi < lo) {   // off: the vectors go
    ctx->xcOn = ctx->xcDirty = false;
    ctx->xcLo = 0;
    ctx->xcHi = -1;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    ctx->xcPlus.release();
    ctx->xcMinus.release();
    return GX_OK;
  }
  const int oldLo = ctx->xcLo, oldHi = ctx->xcHi;
  ctx->xcLo = lo;
  ctx->xcHi = hi;
  if (int rc = xc_layout(ctx)) {   // (a refused setting leaves the old one)
    ctx->xcLo = oldLo;
    ctx->xcHi = oldHi;
    return rc;
  }
  ctx->xcOn = true;
  return GX_OK;
}

int gx_push_tags(gx_ctx* ctx, const gx_tag* tags, size_t n) {
  if (!ctx || !ctx->xcOn || (ctx->phase != 1 && ctx->phase != 3) || (n && !tags)) return GX_ERR_ORDER;
  if (!n) return GX_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  return xc_push(ctx, tags, n);
}

int gx_xcor_samples(gx_ctx* ctx, int* n_samples) {
  if (!ctx || !n_samples) return GX_ERR_ORDER;
  *n_samples = (int)ctx->xc.size();
  return GX_OK;
}

int gx_get_xcor(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, uint64_t* n_pos, uint64_t* n_plus, uint64_t* n_minus, uint64_t* rejected, int* lo,
                int* hi, uint64_t* n11, size_t cap) {
  if (!ctx || sample < 0 || (size_t)sample >= ctx->xc.size()) return GX_ERR_ORDER;
  return xc_give(ctx->xc[sample], ctx->xcLo, ctx->xcHi, rep, is_ctrl, n_pos, n_plus, n_minus, rejected, lo, hi, n11, cap);
}

int gx_xcor_group(gx_ctx* const* ctxs, int n_ctx, int sample, int* rep, int* is_ctrl, uint64_t* n_pos, uint64_t* n_plus, uint64_t* n_minus,
                  uint64_t* rejected, int* lo, int* hi, uint64_t* n11, size_t cap) {
  gx_ctx::XcResult sum;
  if (int rc = xc_sum(ctxs, n_ctx, sample, sum)) return rc;
  return xc_give(sum, ctxs[0]->xcLo, ctxs[0]->xcHi, rep, is_ctrl, n_pos, n_plus, n_minus, rejected, lo, hi, n11, cap);
}

int gx_xcor_tags(gx_ctx* ctx, const uint32_t* lens, int n_chrom, const gx_tag* tags, size_t n, int lo, int hi, unsigned grid, uint32_t tile_words,
                 uint64_t* n_pos, uint64_t* n_plus, uint64_t* n_minus, uint64_t* rejected, uint64_t* n11, size_t cap) {
  if (!ctx || !lens || n_chrom < 1 || (n && !tags) || (cap && !n11)) return GX_ERR_ORDER;
  if (int rc = guard_closed(ctx, "gx_xcor_tags")) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  gx_ctx::XcResult r;
  if (int rc = xc_tags(ctx, lens, n_chrom, tags, n, lo, hi, grid, tile_words, r)) return rc;
  return xc_give(r, lo, hi, nullptr, nullptr, n_pos, n_plus, n_minus, rejected, nullptr, nullptr, n11, cap);
}

int gx_xcor_geometry(int* lanes, int* grid, uint32_t* tile_words, uint32_t* pad_words_for_4096, uint64_t* flush_words) {
  static_assert(XC_MAX_SHIFT == GX_XCOR_MAX_SHIFT && XC_MIN_TILE == GX_XCOR_MIN_TILE, "the header's limits are the kernel's");
  if (lanes) *lanes = (int)XC_NT;
  if (grid) *grid = (int)XC_GRID;
  if (tile_words) *tile_words = XC_TILE;
  if (pad_words_for_4096) *pad_words_for_4096 = xc_pad_words(-XC_MAX_SHIFT, XC_MAX_SHIFT);
  if (flush_words) *flush_words = XC_FLUSH_WORDS;
  return GX_OK;
}

int gx_write_xcor_group(gx_ctx* const* ctxs, int n_ctx, int read_len, FILE* curve, FILE* metrics) {
  if (!ctxs || n_ctx < 1 || !ctxs[0] || (!curve && !metrics)) return GX_ERR_ORDER;
  const int nS = (int)ctxs[0]->xc.size();
  if (nS < 1) return GX_ERR_ORDER;
  const int lo = ctxs[0]->xcLo, hi = ctxs[0]->xcHi;
  std::vector<gx_ctx::XcResult> sums((size_t)nS);   // (each sample summed once; the writers read the sums in place)
  std::vector<int> rep, ctrl;
  std::vector<uint64_t> N, nP, nM, rej;
  std::vector<const uint64_t*> pc;
  for (int i = 0; i < nS; i++) {
    const gx_ctx::XcResult& r = sums[i];
    if (int rc = xc_sum(ctxs, n_ctx, i, sums[i])) return rc;
    rep.push_back(r.rep); ctrl.push_back(r.ctrl); N.push_back(r.N); nP.push_back(r.nP); nM.push_back(r.nM); rej.push_back(r.rejected);
    pc.push_back(r.n11.data());
  }
  if (curve)
    if (int rc = gx_format_xcor(curve, nS, rep.data(), ctrl.data(), N.data(), nP.data(), nM.data(), rej.data(), lo, hi, pc.data())) return rc;
  if (metrics)
    if (int rc = gx_format_xcor_metrics(metrics, nS, rep.data(), ctrl.data(), N.data(), nP.data(), nM.data(), lo, hi, pc.data(), read_len)) return rc;
  return GX_OK;
}

int gx_set_genome(gx_ctx* ctx, int on) {
  if (!ctx || ctx->nChrom == 0) return GX_ERR_ORDER;   // the table is known
  if (int rc = guard_closed(ctx, "gx_set_genome")) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  drop_gcbias(ctx);
  if (!on) {   // off: the vectors go
    ctx->gcOn = ctx->gcDirty = false;
    ctx->gcVec.release();
    ctx->gcAcgt.release();
    ctx->gcAg.release();
    ctx->seqOn = false;
    ctx->gcDir.release();
    ctx->gcPushed.clear();
    return GX_OK;
  }
  if (int rc = gc_layout(ctx)) return rc;
  ctx->gcOn = true;
  return GX_OK;
}

int gx_push_sequence(gx_ctx* ctx, int chrom, uint64_t first_base, const char* bases, size_t n) {
  if (!ctx || !ctx->gcOn || (n && !bases)) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  return gc_push(ctx, chrom, first_base, bases, n);
}

int gx_genome_info(gx_ctx* ctx, uint64_t* bases_pushed, uint64_t* gc, uint64_t* acgt) {
  if (!ctx || !ctx->gcOn) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  if (int rc = gc_current(ctx)) return rc;
  std::vector<gx_region> reg;
  uint64_t pushed = 0;
  for (u32 c = 0; c < ctx->nChrom; c++) {
    pushed += ctx->gcPushed[c];
    if (ctx->gcChrom[c].laid) reg.push_back(gx_region{c, 0, ctx->gcChrom[c].len});
  }
  std::vector<uint64_t> g(reg.size() + 1, 0), a(reg.size() + 1, 0);
  if (int rc = gc_content(ctx, reg.data(), reg.size(), g.data(), a.data())) return rc;
  uint64_t sg = 0, sa = 0;
  for (size_t i = 0; i < reg.size(); i++) {
    sg += g[i];
    sa += a[i];
  }
  if (bases_pushed) *bases_pushed = pushed;
  if (gc) *gc = sg;
  if (acgt) *acgt = sa;
  return GX_OK;
}

int gx_gc_content(gx_ctx* ctx, const gx_region* regions, size_t n, uint64_t* gc, uint64_t* acgt) {
  if (!ctx || !ctx->gcOn || (n && (!regions || !gc || !acgt))) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  return gc_content(ctx, regions, n, gc, acgt);
}

int gx_gc_bias(gx_ctx* ctx, int window, int* n_samples) {
  if (!ctx) return GX_ERR_ORDER;
  if (!ctx->gcOn) return refuse(ctx, "gx_gc_bias needs the genome (gx_set_genome)");
  if (int rc = guard_kept(ctx, "gx_gc_bias", true)) return rc;
  if (int rc = gc_check_window(ctx, window)) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  ctx->gcReady = false;
  if (int rc = gc_bias_kept(ctx, (u32)window)) return rc;
  if (n_samples) *n_samples = (int)ctx->gcRes.size();
  return GX_OK;
}

int gx_get_gc_bias(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, int* window, uint64_t* F, uint64_t* f_unclassed, uint64_t* Nn, uint64_t* Nw,
                   uint64_t* n_unclassed, uint64_t* w_unclassed, size_t cap) {
  if (!ctx || !ctx->gcReady || sample < 0 || (size_t)sample >= ctx->gcRes.size()) return GX_ERR_ORDER;
  return gc_give(ctx->gcRes[sample], rep, is_ctrl, window, F, f_unclassed, Nn, Nw, n_unclassed, w_unclassed, cap);
}

int gx_gc_bias_group(gx_ctx* const* ctxs, int n_ctx, int sample, int* rep, int* is_ctrl, int* window, uint64_t* F, uint64_t* f_unclassed, uint64_t* Nn,
                     uint64_t* Nw, uint64_t* n_unclassed, uint64_t* w_unclassed, size_t cap) {
  gx_ctx::GcResult sum;
  if (int rc = gc_sum(ctxs, n_ctx, sample, sum)) return rc;
  return gc_give(sum, rep, is_ctrl, window, F, f_unclassed, Nn, Nw, n_unclassed, w_unclassed, cap);
}

int gx_gc_bias_events(gx_ctx* ctx, const void* ev, size_t n, int packed, int window, unsigned grid_expected, uint32_t tile_words, uint64_t flush_words,
                      unsigned grid_observed, uint64_t* F, uint64_t* f_unclassed, uint64_t* Nn, uint64_t* Nw, uint64_t* n_unclassed,
                      uint64_t* w_unclassed, size_t cap) {
  if (!ctx || !ctx->gcOn || (n && !ev) || (cap && (!F || !Nn || !Nw))) return GX_ERR_ORDER;
  if (int rc = guard_closed(ctx, "gx_gc_bias_events")) return rc;
  if (int rc = gc_check_window(ctx, window)) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  gx_ctx::GcResult r;
  if (int rc = gc_bias_events(ctx, ev, n, packed != 0, (u32)window, grid_expected, tile_words, flush_words, grid_observed, r)) return rc;
  return gc_give(r, nullptr, nullptr, nullptr, F, f_unclassed, Nn, Nw, n_unclassed, w_unclassed, cap);
}

int gx_gc_geometry(int* lanes, int* grid, uint32_t* tile_words, uint32_t* min_tile_words, uint32_t* pad_words, uint32_t* block_bases,
                   uint64_t* flush_words) {
  static_assert(GC_MAX_WINDOW == GX_GC_MAX_WINDOW && GC_MIN_TILE == GX_GC_MIN_TILE, "the header's limits are the kernel's");
  if (lanes) *lanes = (int)GC_NT;
  if (grid) *grid = (int)GC_GRID;
  if (tile_words) *tile_words = GC_TILE;
  if (min_tile_words) *min_tile_words = GC_MIN_TILE;
  if (pad_words) *pad_words = GC_PAD;
  if (block_bases) *block_bases = GC_BLOCK_WORDS * 64;
  if (flush_words) *flush_words = GC_FLUSH_WORDS;
  return GX_OK;
}

int gx_write_gc_bias_group(gx_ctx* const* ctxs, int n_ctx, int window, FILE* out) {
  if (!ctxs || n_ctx < 1 || !ctxs[0] || !out) return GX_ERR_ORDER;
  int nS = 0;
  if (int rc = pass_on_all(ctxs, n_ctx, [&](gx_ctx* c, int* n) { return gx_gc_bias(c, window, n); }, &nS)) return rc;
  std::vector<gx_ctx::GcResult> sums((size_t)nS);   // (each sample summed once; the writer reads the sums in place)
  std::vector<int> rep, ctrl;
  std::vector<uint64_t> fUn, nUn, wUn;
  std::vector<const uint64_t*> pF, pN, pW;
  for (int i = 0; i < nS; i++) {
    const gx_ctx::GcResult& r = sums[i];
    if (int rc = gc_sum(ctxs, n_ctx, i, sums[i])) return rc;
    rep.push_back(r.rep); ctrl.push_back(r.ctrl); fUn.push_back(r.fUn); nUn.push_back(r.nUn); wUn.push_back(r.wUn);
    pF.push_back(r.F.data()); pN.push_back(r.Nn.data()); pW.push_back(r.Nw.data());
  }
  return gx_format_gc_bias(out, nS, rep.data(), ctrl.data(), window, pF.data(), fUn.data(), pN.data(), pW.data(), nUn.data(), wUn.data());
}

int gx_write_gc_peaks_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, FILE* out) {
  if (!ctxs || n_ctx < 1 || !names || !out) return GX_ERR_ORDER;
  gx_peak_merge::Merged m;
  if (int rc = gx_peak_merge::merged_peaks(ctxs, n_ctx, m)) return rc;
  // each context on its own peaks (it holds their chromosomes' bases), which are merged peaks rank[first[g] ..]
  std::vector<uint64_t> gc(m.size()), acgt(m.size());
  for (int g = 0; g < n_ctx; g++) {
    std::vector<gx_region> own;
    for (size_t j = m.first[g]; j < m.first[g + 1]; j++) own.push_back(m.regions[m.rank[j]]);
    if (int rc = gx_gc_content(ctxs[g], own.data(), own.size(), gc.data() + m.first[g], acgt.data() + m.first[g])) return rc;
  }
  gc = permuted(m, gc);
  acgt = permuted(m, acgt);
  return gx_format_gc_peaks(out, names, m.regions.data(), m.size(), gc.data(), acgt.data());
}

int gx_set_genome_bases(gx_ctx* ctx, int on) {
  if (!ctx) return GX_ERR_ORDER;
  if (int rc = guard_closed(ctx, "gx_set_genome_bases")) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  return seq_set_bases(ctx, on != 0);
}

int gx_get_sequence(gx_ctx* ctx, int chrom, uint64_t start, size_t n, char* out) {
  if (!ctx || !ctx->gcOn || (n && !out)) return GX_ERR_ORDER;
  HIPCHECK(hipSetDevice(ctx->device));
  return seq_get(ctx, chrom, start, n, out);
}

int gx_set_motifs(gx_ctx* ctx, const gx_motif* m, int n, const int16_t* scores) {
  if (!ctx || (n > 0 && (!m || !scores))) return GX_ERR_ORDER;
  return mot_set(ctx, m, n, scores);
}

int gx_motif_scan_regions(gx_ctx* ctx, const gx_region* regions, size_t n, unsigned grid, uint32_t step_words, uint32_t batch_motifs, size_t list_cap,
                          gx_motif_hit* out, size_t cap, size_t* n_out, uint64_t* windows, uint64_t* hits_fwd, uint64_t* hits_rev) {
  if (!ctx || (n && !regions) || (cap && !out)) return GX_ERR_ORDER;
  if (!ctx->seqOn) return refuse(ctx, "gx_motif_scan_regions needs the bases (gx_set_genome_bases)");
  if (int rc = guard_closed(ctx, "gx_motif_scan_regions")) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  std::vector<gx_motif_hit> hits;
  std::vector<uint64_t> counts;
  if (int rc = mot_pass(ctx, regions, n, MotGeometry{grid, step_words, batch_motifs, (u64)list_cap}, hits, counts)) return rc;
  if (n_out) *n_out = hits.size();
  if (const size_t k = std::min(cap, hits.size())) memcpy(out, hits.data(), k * sizeof(gx_motif_hit));
  return windows || hits_fwd || hits_rev ? mot_give(counts, ctx->motMeta.size(), windows, hits_fwd, hits_rev, ctx->motMeta.size()) : GX_OK;
}

int gx_motif_scan_peaks(gx_ctx* ctx, size_t* n_hits) {
  if (!ctx) return GX_ERR_ORDER;
  if (!ctx->seqOn) return refuse(ctx, "gx_motif_scan_peaks needs the bases (gx_set_genome_bases)");
  if (ctx->phase != 0 || !ctx->peaksReady) return refuse(ctx, "gx_motif_scan_peaks comes after gx_find_peaks, with no sample open");
  HIPCHECK(hipSetDevice(ctx->device));
  if (int rc = mot_scan_peaks(ctx)) return rc;
  if (n_hits) *n_hits = ctx->motHits.size();
  return GX_OK;
}

int gx_get_motif_hits(gx_ctx* ctx, gx_motif_hit* out, size_t cap) {
  if (!ctx || !ctx->motReady || (cap && !out)) return GX_ERR_ORDER;
  if (const size_t k = std::min(cap, ctx->motHits.size())) memcpy(out, ctx->motHits.data(), k * sizeof(gx_motif_hit));
  return GX_OK;
}

int gx_get_motif_counts(gx_ctx* ctx, uint64_t* windows, uint64_t* hits_fwd, uint64_t* hits_rev, size_t cap) {
  if (!ctx || !ctx->motReady) return GX_ERR_ORDER;
  return mot_give(ctx->motCounts, ctx->motMeta.size(), windows, hits_fwd, hits_rev, cap);
}

int gx_motif_last(gx_ctx* ctx, uint32_t* reruns, uint32_t* batches) {
  if (!ctx) return GX_ERR_ORDER;
  if (reruns) *reruns = ctx->motLastReruns;
  if (batches) *batches = ctx->motLastBatches;
  return GX_OK;
}

int gx_motif_scan_genome(gx_ctx* ctx, uint64_t* windows, uint64_t* hits_fwd, uint64_t* hits_rev, size_t cap) {
  return gx_motif_scan_genome_group(&ctx, 1, windows, hits_fwd, hits_rev, cap);
}

// Every context's pass is launched, with its read-back queued on its stream, before the first is waited for: with several devices
// the passes run side by side.
int gx_motif_scan_genome_group(gx_ctx* const* ctxs, int n_ctx, uint64_t* windows, uint64_t* hits_fwd, uint64_t* hits_rev, size_t cap) {
  if (!ctxs || n_ctx < 1 || !ctxs[0]) return GX_ERR_ORDER;
  std::vector<MotRun> runs((size_t)n_ctx);
  for (int g = 0; g < n_ctx; g++) {
    gx_ctx* ctx = ctxs[g];
    if (!ctx || ctx->motMeta.size() != ctxs[0]->motMeta.size()) return GX_ERR_ORDER;
    if (!ctx->seqOn) return refuse(ctx, "gx_motif_scan_genome needs the bases (gx_set_genome_bases)");
    if (int rc = guard_closed(ctx, "gx_motif_scan_genome")) return rc;
  }
  int bad = GX_OK;
  for (int g = 0; g < n_ctx && !bad; g++) {
    gx_ctx* ctx = ctxs[g];
    HIPCHECK(hipSetDevice(ctx->device));
    if (int rc = gc_current(ctx)) return rc;
    const std::vector<gx_region> reg = mot_genome_regions(ctx);
    bad = mot_count_begin(ctx, reg.data(), reg.size(), runs[(size_t)g]);
  }
  std::vector<uint64_t> sum, counts;
  for (int g = 0; g < n_ctx; g++) {   // (every pass that was launched is drained, also behind a failure: its buffers are the run's)
    gx_ctx* ctx = ctxs[g];
    HIPCHECK(hipSetDevice(ctx->device));
    if (int rc = mot_count_end(ctx, runs[(size_t)g], counts)) return rc;
    if (g == 0) sum = counts;
    else
      for (size_t k = 0; k < sum.size(); k++) sum[k] += counts[k];
  }
  if (bad) return bad;
  return mot_give(sum, ctxs[0]->motMeta.size(), windows, hits_fwd, hits_rev, cap);
}

int gx_motif_grid(uint64_t units, uint32_t step_words, unsigned grid, unsigned* chosen) {
  unsigned g = 0;
  const char* why = "";
  if (int rc = mot_grid(units, step_words ? step_words : MOT_STEP, grid, &g, &why)) return rc;
  if (chosen) *chosen = g;
  return GX_OK;
}

int gx_motif_geometry(int* lanes, int* grid, uint32_t* positions_per_step, uint32_t* step_words, uint32_t* batch_motifs, size_t* list_cap,
                      uint64_t* flush_runs) {
  if (lanes) *lanes = (int)MOT_NT;
  if (grid) *grid = (int)MOT_GRID;
  if (positions_per_step) *positions_per_step = 64;
  if (step_words) *step_words = MOT_STEP;
  if (batch_motifs) *batch_motifs = MOT_BATCH;
  if (list_cap) *list_cap = (size_t)MOT_LIST_MIN;
  if (flush_runs) *flush_runs = MOT_FLUSH_RUNS;
  return GX_OK;
}

// every context's scan of its peaks (run where the context does not hold it), the hits on the merged peaks, the counts added
static int motif_group(gx_ctx* const* ctxs, int n_ctx, int n_motifs, gx_peak_merge::Merged& m, std::vector<gx_motif_hit>& hits,
                       std::vector<uint64_t>& cPeaks) {
  if (!ctxs || n_ctx < 1 || n_motifs < 0) return GX_ERR_ORDER;
  cPeaks.assign(3 * (size_t)n_motifs, 0);
  for (int g = 0; g < n_ctx; g++) {
    if (!ctxs[g] || ctxs[g]->motMeta.size() != (size_t)n_motifs) return GX_ERR_ORDER;
    if (!ctxs[g]->motReady)   // (else the context holds the scan of these peaks with these motifs: nothing runs again)
      if (int rc = gx_motif_scan_peaks(ctxs[g], nullptr)) return rc;
    for (size_t i = 0; i < cPeaks.size(); i++) cPeaks[i] += ctxs[g]->motCounts[i];
  }
  if (int rc = gx_peak_merge::merged_peaks(ctxs, n_ctx, m)) return rc;
  std::vector<std::vector<gx_motif_hit>> own;
  for (int g = 0; g < n_ctx; g++) own.push_back(ctxs[g]->motHits);
  hits = renumbered(m, own, &gx_motif_hit::region, gx_peak_merge::motif_hit_less);
  return GX_OK;
}

int gx_write_motifs_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, const gx_motif* motifs, const char* const* ids,
                          const char* const* motif_names, const double* p_threshold, int n_motifs, FILE* hits_out, FILE* summary_out,
                          uint64_t* counts_peaks, uint64_t* counts_genome, gx_motif_report* report) {
  if (!hits_out && !summary_out) return GX_ERR_ORDER;
  gx_peak_merge::Merged m;
  std::vector<gx_motif_hit> hits;
  std::vector<uint64_t> cP;
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = motif_group(ctxs, n_ctx, n_motifs, m, hits, cP)) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  const size_t nM = (size_t)n_motifs;
  std::vector<uint64_t> cG(3 * nM, 0);
  std::vector<uint32_t> summit;
  for (const gx_peak& p : m.peaks) summit.push_back(p.summit);
  if (summary_out)
    if (int rc = gx_motif_scan_genome_group(ctxs, n_ctx, cG.data(), cG.data() + nM, cG.data() + 2 * nM, nM)) return rc;
  const auto t2 = std::chrono::steady_clock::now();
  if (hits_out)
    if (int rc = gx_format_motif_hits(hits_out, names, m.regions.data(), summit.data(), m.size(), motifs, ids, motif_names, p_threshold, n_motifs, hits.data(), hits.size()))
      return rc;
  if (summary_out)
    if (int rc = gx_format_motif_summary(summary_out, m.regions.data(), m.size(), motifs, ids, motif_names, p_threshold, n_motifs, hits.data(), hits.size(), cP.data(), cG.data()))
      return rc;
  if (counts_peaks) std::copy(cP.begin(), cP.end(), counts_peaks);
  if (counts_genome) std::copy(cG.begin(), cG.end(), counts_genome);
  if (report) {
    report->hits = hits.size();
    report->peaks_with_hit = 0;
    for (size_t i = 0; i < hits.size(); i++) report->peaks_with_hit += i == 0 || hits[i].region != hits[i - 1].region;
    report->peaks_seconds = std::chrono::duration<double>(t1 - t0).count();
    report->genome_seconds = std::chrono::duration<double>(t2 - t1).count();
  }
  return GX_OK;
}

int gx_write_motif_hits_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, const gx_motif* motifs, const char* const* ids,
                              const char* const* motif_names, const double* p_threshold, int n_motifs, FILE* out) {
  return gx_write_motifs_group(ctxs, n_ctx, names, motifs, ids, motif_names, p_threshold, n_motifs, out, nullptr, nullptr, nullptr, nullptr);
}

int gx_write_motif_summary_group(gx_ctx* const* ctxs, int n_ctx, const gx_motif* motifs, const char* const* ids, const char* const* motif_names,
                                 const double* p_threshold, int n_motifs, FILE* out) {
  return gx_write_motifs_group(ctxs, n_ctx, nullptr, motifs, ids, motif_names, p_threshold, n_motifs, nullptr, out, nullptr, nullptr, nullptr);
}

// ---- every k-mer of the peaks and of the genome counted (gx_kmers.h, gx_host_kmers.h) ----
static int kmer_guard(gx_ctx* ctx, const char* fn, int k) {
  if (!ctx->seqOn) return refuse(ctx, std::string(fn) + " needs the bases (gx_set_genome_bases)");
  if (int rc = guard_closed(ctx, fn)) return rc;
  return kmer_check_k(ctx, k);
}

int gx_kmer_count_regions(gx_ctx* ctx, const gx_region* regions, size_t n, int k, unsigned grid, uint32_t step_words, uint64_t flush_runs,
                          uint64_t* counts, uint64_t* windows) {
  if (!ctx || (n && !regions)) return GX_ERR_ORDER;
  if (int rc = kmer_guard(ctx, "gx_kmer_count_regions", k)) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  std::vector<uint64_t> c;
  u64 w = 0;
  if (int rc = kmer_pass(ctx, regions, n, (u32)k, KmerGeometry{grid, step_words, flush_runs}, c, &w, nullptr)) return rc;
  if (counts) std::copy(c.begin(), c.end(), counts);
  if (windows) *windows = w;
  return GX_OK;
}

int gx_kmer_count_peaks(gx_ctx* ctx, int k, int flank, uint64_t* windows, uint64_t* regions_counted) {
  if (!ctx) return GX_ERR_ORDER;
  if (int rc = kmer_guard(ctx, "gx_kmer_count_peaks", k)) return rc;
  if (ctx->phase != 0 || !ctx->peaksReady) return refuse(ctx, "gx_kmer_count_peaks comes after gx_find_peaks, with no sample open");
  HIPCHECK(hipSetDevice(ctx->device));
  if (int rc = kmer_count_peaks(ctx, (u32)k, flank)) return rc;
  if (windows) *windows = ctx->kmWindows;
  if (regions_counted) *regions_counted = ctx->kmRegions;
  return GX_OK;
}

int gx_get_kmer_counts(gx_ctx* ctx, uint64_t* counts, size_t cap) {
  if (!ctx || !ctx->kmReady || (cap && !counts)) return GX_ERR_ORDER;
  if (const size_t n = std::min(cap, ctx->kmCounts.size())) std::copy(ctx->kmCounts.begin(), ctx->kmCounts.begin() + n, counts);
  return GX_OK;
}

int gx_kmer_count_genome(gx_ctx* ctx, int k, uint64_t* counts, size_t cap, uint64_t* windows) {
  return gx_kmer_count_genome_group(&ctx, 1, k, counts, cap, windows);
}

// Every context's pass is launched, with its read-back queued on its stream, before the first is waited for (as
// gx_motif_scan_genome_group).
int gx_kmer_count_genome_group(gx_ctx* const* ctxs, int n_ctx, int k, uint64_t* counts, size_t cap, uint64_t* windows) {
  if (!ctxs || n_ctx < 1 || !ctxs[0] || (cap && !counts)) return GX_ERR_ORDER;
  std::vector<KmerRun> runs((size_t)n_ctx);
  for (int g = 0; g < n_ctx; g++) {
    if (!ctxs[g]) return GX_ERR_ORDER;
    if (int rc = kmer_guard(ctxs[g], "gx_kmer_count_genome", k)) return rc;
  }
  int bad = GX_OK;
  for (int g = 0; g < n_ctx && !bad; g++) {
    gx_ctx* ctx = ctxs[g];
    HIPCHECK(hipSetDevice(ctx->device));
    if (int rc = gc_current(ctx)) return rc;
    const std::vector<gx_region> reg = mot_genome_regions(ctx);
    bad = kmer_begin(ctx, reg.data(), reg.size(), (u32)k, KmerGeometry{0, 0, 0}, runs[(size_t)g]);
  }
  std::vector<uint64_t> sum, c;
  u64 wSum = 0;
  for (int g = 0; g < n_ctx; g++) {   // (every pass that was launched is drained, also behind a failure: its buffers are the run's)
    gx_ctx* ctx = ctxs[g];
    HIPCHECK(hipSetDevice(ctx->device));
    u64 w = 0;
    if (int rc = kmer_end(ctx, runs[(size_t)g], c, &w)) return rc;
    wSum += w;
    if (sum.empty()) sum.assign((size_t)1 << (2 * k), 0);
    for (size_t i = 0; i < sum.size() && i < c.size(); i++) sum[i] += c[i];
  }
  if (bad) return bad;
  if (const size_t n = std::min(cap, sum.size())) std::copy(sum.begin(), sum.begin() + n, counts);
  if (windows) *windows = wSum;
  return GX_OK;
}

int gx_kmer_last(gx_ctx* ctx, int* path, uint32_t* flushes) {
  if (!ctx) return GX_ERR_ORDER;
  if (path) *path = (int)ctx->kmLastPath;
  if (flushes) *flushes = ctx->kmLastFlushes;
  return GX_OK;
}

int gx_kmer_force_hbm(gx_ctx* ctx, int on) {
  if (!ctx) return GX_ERR_ORDER;
  ctx->kmForceHbm = on != 0;
  return GX_OK;
}

int gx_kmer_geometry(int* lanes, int* grid, uint32_t* positions_per_step, uint32_t* step_words, uint64_t* flush_runs, int* max_k, int* lds_max_k) {
  if (lanes) *lanes = (int)MOT_NT;
  if (grid) *grid = (int)MOT_GRID;
  if (positions_per_step) *positions_per_step = 64;
  if (step_words) *step_words = MOT_STEP;
  if (flush_runs) *flush_runs = KMER_FLUSH_RUNS;
  if (max_k) *max_k = (int)KMER_MAX_K;
  if (lds_max_k) *lds_max_k = (int)KMER_LDS_MAX_K;
  return GX_OK;
}

// --kmers' table over the contexts of a run: one count of every context's peaks, one genome pass launched on every context
// before the first is waited for, the counts added
int gx_write_kmers_group(gx_ctx* const* ctxs, int n_ctx, int k, int flank, int top, FILE* out, gx_kmer_report* report) {
  if (!ctxs || n_ctx < 1 || !ctxs[0] || !out || top < 0) return GX_ERR_ORDER;
  if (k < 1 || k > (int)KMER_MAX_K) return refuse(ctxs[0], "kmers: k must satisfy 1 <= k <= 12");
  const size_t nT = (size_t)1 << (2 * k);
  std::vector<uint64_t> cP(nT, 0), cG(nT, 0);
  uint64_t wP = 0, wG = 0, nReg = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int g = 0; g < n_ctx; g++) {
    if (!ctxs[g]) return GX_ERR_ORDER;
    uint64_t w = 0, r = 0;
    if (int rc = gx_kmer_count_peaks(ctxs[g], k, flank, &w, &r)) return rc;
    wP += w;
    nReg += r;
    for (size_t i = 0; i < nT; i++) cP[i] += ctxs[g]->kmCounts[i];
  }
  const auto t1 = std::chrono::steady_clock::now();
  if (int rc = gx_kmer_count_genome_group(ctxs, n_ctx, k, cG.data(), nT, &wG)) return rc;
  const auto t2 = std::chrono::steady_clock::now();
  if (int rc = gx_format_kmers(out, k, flank, nReg, wP, wG, cP.data(), cG.data(), top)) return rc;
  if (report) {
    *report = gx_kmer_report{};
    report->windows_peaks = wP;
    report->windows_genome = wG;
    report->regions_counted = nReg;
    size_t n = 0;
    if (int rc = gx_kmer_stats(k, cP.data(), wP, cG.data(), wG, nullptr, 0, &n)) return rc;
    report->kmers_counted = n;
    std::vector<gx_kmer_row> rows(std::max<size_t>(n, 1));
    if (int rc = gx_kmer_stats(k, cP.data(), wP, cG.data(), wG, rows.data(), n, nullptr)) return rc;
    report->n_top = (int)std::min<size_t>(n, 3);
    for (int i = 0; i < report->n_top; i++) {
      report->top_code[i] = rows[(size_t)i].code;
      report->top_z[i] = rows[(size_t)i].z;
    }
    report->peaks_seconds = std::chrono::duration<double>(t1 - t0).count();
    report->genome_seconds = std::chrono::duration<double>(t2 - t1).count();
  }
  return GX_OK;
}

uint32_t gx_subsample_draw(uint64_t seed, uint32_t sample, uint64_t index) { return subsample_draw(subsample_key(seed, sample), index); }

int gx_subsample_geometry(int* lanes, int* grid, uint32_t* block_events) {
  if (lanes) *lanes = SUB_NT;
  if (grid) *grid = (int)SUB_GRID;
  if (block_events) *block_events = SUB_BLOCK;
  return GX_OK;
}

int gx_subsample_events(gx_ctx* ctx, const void* ev, size_t n, int packed, uint64_t seed, uint32_t sample, uint64_t threshold, unsigned grid,
                        gx_event* out, size_t cap, size_t* n_out) {
  if (!ctx || (n && !ev) || (cap && !out)) return GX_ERR_ORDER;
  if (int rc = guard_closed(ctx, "gx_subsample_events")) return rc;
  if (threshold > ((u64)1 << 32)) return refuse(ctx, "subsample: a threshold above 2^32");
  if (grid > SUB_MAX_GRID) return refuse(ctx, "subsample: more than 65535 workgroups");
  HIPCHECK(hipSetDevice(ctx->device));
  std::vector<gx_ctx::Seg> segs;
  if (int rc = kept_upload(ctx, ev, n, packed != 0, segs)) return rc;
  const CntChunk* dCk = nullptr;
  const u64* dFirst = nullptr;
  u32 nCk = 0;
  u64 nEv = 0, nKept = 0;
  if (int rc = sub_stage(ctx, segs, &dCk, &dFirst, &nCk, &nEv)) return rc;
  if (int rc = sub_pass(ctx, dCk, dFirst, nCk, nEv, subsample_key(seed, sample), threshold, grid, ctx->subOut, &nKept)) return rc;
  return sub_give(ctx, ctx->subOut, nKept, out, cap, n_out);
}

int gx_subsample_kept(gx_ctx* ctx, int sample, uint64_t seed, uint64_t threshold, gx_event* out, size_t cap, size_t* n_out) {
  if (!ctx || (cap && !out)) return GX_ERR_ORDER;
  if (int rc = guard_kept(ctx, "gx_subsample_kept", false)) return rc;
  if (int rc = guard_closed(ctx, "gx_subsample_kept")) return rc;
  if (sample < 0 || (size_t)sample >= ctx->kept.size()) return refuse(ctx, "gx_subsample_kept: no such sample");
  if (threshold > ((u64)1 << 32)) return refuse(ctx, "subsample: a threshold above 2^32");
  HIPCHECK(hipSetDevice(ctx->device));
  u64 n = 0, nKept = 0;
  if (int rc = sub_kept(ctx, (size_t)sample, seed, threshold, &n, &nKept)) return rc;
  return sub_give(ctx, ctx->subBufs[sample], nKept, out, cap, n_out);
}

int gx_saturation(gx_ctx* ctx, const uint64_t* threshold, int n_points, uint64_t seed, unsigned flags, gx_sat_point* out) {
  if (!ctx || !threshold || n_points < 1 || !out || (flags & ~GX_SAT_CONTROLS)) return GX_ERR_ORDER;
  if (int rc = guard_kept(ctx, "gx_saturation", false)) return rc;
  if (ctx->phase != 0 || !ctx->peaksReady) return refuse(ctx, "gx_saturation comes after gx_find_peaks, with no sample open");
  if (ctx->world > 1 || ctx->forceColl) return refuse(ctx, "gx_saturation: one context only (the re-call on several needs collectives between their children)");
  for (int j = 0; j < n_points; j++)
    if (threshold[j] > ((u64)1 << 32)) return refuse(ctx, "subsample: a threshold above 2^32");
  HIPCHECK(hipSetDevice(ctx->device));
  if (int rc = sat_child(ctx)) return rc;
  std::vector<gx_sat_point> pts((size_t)n_points);
  std::vector<std::vector<gx_peak>> peaks((size_t)n_points);
  for (int j = 0; j < n_points; j++)
    if (int rc = sat_point(ctx, threshold[j], seed, flags, pts[j], peaks[j])) return rc;
  std::copy(pts.begin(), pts.end(), out);
  ctx->satPts = std::move(pts);
  ctx->satPeaks = std::move(peaks);
  return GX_OK;
}

int gx_get_saturation_peaks(gx_ctx* ctx, int point, gx_peak* out, size_t cap) {
  if (!ctx || point < 0 || (size_t)point >= ctx->satPeaks.size() || (cap && !out)) return GX_ERR_ORDER;
  const size_t n = std::min(cap, ctx->satPeaks[point].size());
  if (n) memcpy(out, ctx->satPeaks[point].data(), n * sizeof(gx_peak));
  return GX_OK;
}

int gx_write_saturation(gx_ctx* ctx, FILE* out) {
  if (!ctx || !out || ctx->satPts.empty() || !ctx->peaksReady) return GX_ERR_ORDER;
  const size_t nP = ctx->satPts.size();
  const gx_peak* full = static_cast<const gx_peak*>(ctx->hPeaks.p);
  std::vector<uint64_t> rec(nP, 0), sub(nP, 0), bp(nP, 0);
  for (size_t j = 0; j < nP; j++)
    if (int rc = gx_saturation_overlap(full, ctx->nHostPeaks, ctx->satPeaks[j].data(), ctx->satPeaks[j].size(), &rec[j], &sub[j], &bp[j])) return rc;
  return gx_format_saturation(out, (int)nP, ctx->satPts.data(), rec.data(), sub.data(), bp.data(), ctx->nHostPeaks, ctx->peakBP);
}

int gx_subsample_split_events(gx_ctx* ctx, const void* ev, size_t n, int packed, uint64_t seed, uint32_t sample, uint64_t threshold,
                              unsigned grid, gx_event* out, size_t cap, size_t* n_a) {
  if (!ctx || (n && !ev) || (cap && !out)) return GX_ERR_ORDER;
  if (int rc = guard_closed(ctx, "gx_subsample_split_events")) return rc;
  if (threshold > ((u64)1 << 32)) return refuse(ctx, "subsample: a threshold above 2^32");
  if (grid > SUB_MAX_GRID) return refuse(ctx, "subsample: more than 65535 workgroups");
  HIPCHECK(hipSetDevice(ctx->device));
  std::vector<gx_ctx::Seg> segs;
  if (int rc = kept_upload(ctx, ev, n, packed != 0, segs)) return rc;
  const CntChunk* dCk = nullptr;
  const u64* dFirst = nullptr;
  u32 nCk = 0;
  u64 nEv = 0, nA = 0;
  if (int rc = sub_stage(ctx, segs, &dCk, &dFirst, &nCk, &nEv)) return rc;
  if (int rc = sub_split_pass(ctx, dCk, dFirst, nCk, nEv, subsample_key(seed, sample), threshold, grid, ctx->subOut, &nA)) return rc;
  if (n_a) *n_a = (size_t)nA;
  return sub_give(ctx, ctx->subOut, nEv, out, cap, nullptr);
}

int gx_subsample_split_kept(gx_ctx* ctx, int sample, uint64_t seed, uint64_t threshold, gx_event* out, size_t cap, size_t* n_a) {
  if (!ctx || (cap && !out)) return GX_ERR_ORDER;
  if (int rc = guard_kept(ctx, "gx_subsample_split_kept", false)) return rc;
  if (int rc = guard_closed(ctx, "gx_subsample_split_kept")) return rc;
  if (sample < 0 || (size_t)sample >= ctx->kept.size()) return refuse(ctx, "gx_subsample_split_kept: no such sample");
  if (threshold > ((u64)1 << 32)) return refuse(ctx, "subsample: a threshold above 2^32");
  HIPCHECK(hipSetDevice(ctx->device));
  u64 n = 0, nA = 0;
  if (int rc = sub_split_kept(ctx, (size_t)sample, seed, threshold, &n, &nA)) return rc;
  if (n_a) *n_a = (size_t)nA;
  return sub_give(ctx, ctx->subBufs[sample], n, out, cap, nullptr);
}

int gx_reproducibility(gx_ctx* ctx, uint64_t seed, unsigned flags, gx_repro_call* out, size_t cap, size_t* n_calls) {
  if (!ctx || (cap && !out) || flags) return GX_ERR_ORDER;
  if (int rc = guard_kept(ctx, "gx_reproducibility", false)) return rc;
  if (ctx->phase != 0 || !ctx->peaksReady) return refuse(ctx, "gx_reproducibility comes after gx_find_peaks, with no sample open");
  if (ctx->world > 1 || ctx->forceColl) return refuse(ctx, "gx_reproducibility: one context only (the calls on several need collectives between their children)");
  HIPCHECK(hipSetDevice(ctx->device));
  const int nR = ctx->sample;
  std::vector<ReproRep> reps((size_t)nR);
  for (size_t k = 0; k < ctx->kept.size(); k++) {
    const gx_ctx::KeptSample& ks = ctx->kept[k];
    if (ks.rep < 0 || ks.rep >= nR) continue;
    (ks.ctrl ? reps[ks.rep].kc : reps[ks.rep].kt) = (int)k;
  }
  for (int r = 0; r < nR; r++)
    if (reps[r].kt < 0) return refuse(ctx, "reproducibility: a replicate whose treatment was not kept");
  if (int rc = sat_child(ctx)) return rc;
  for (int r = 0; r < nR; r++)   // each treatment split once: both halves in its own buffer
    if (int rc = sub_split_kept(ctx, (size_t)reps[r].kt, seed, (u64)1 << 31, &reps[r].n, &reps[r].nA)) return rc;
  std::vector<gx_repro_call> calls;
  std::vector<std::vector<ReproPart>> parts;
  for (int r = 0; r < nR; r++) {
    calls.push_back(gx_repro_call{GX_REPRO_ALONE, r, -1, 0, 0, 0, 0});
    parts.push_back({ReproPart{r, -1}});
  }
  for (int r = 0; r < nR; r++)
    for (int h = 0; h < 2; h++) {
      calls.push_back(gx_repro_call{GX_REPRO_SELF, r, h, 0, 0, 0, 0});
      parts.push_back({ReproPart{r, h}});
    }
  for (int h = 0; h < 2; h++) {
    calls.push_back(gx_repro_call{GX_REPRO_POOLED, -1, h, 0, 0, 0, 0});
    parts.emplace_back();
    for (int r = 0; r < nR; r++) parts.back().push_back(ReproPart{r, h});
  }
  std::vector<std::vector<gx_peak>> peaks(calls.size());
  for (size_t i = 0; i < calls.size(); i++)
    if (int rc = repro_call(ctx, reps, parts[i], calls[i], peaks[i])) return rc;
  if (n_calls) *n_calls = calls.size();
  std::copy(calls.begin(), calls.begin() + std::min(cap, calls.size()), out);
  ctx->reproCalls = std::move(calls);
  ctx->reproPeaks = std::move(peaks);
  ctx->reproSeed = seed;
  return GX_OK;
}

int gx_get_reproducibility_peaks(gx_ctx* ctx, int call, gx_peak* out, size_t cap) {
  if (!ctx || call < 0 || (size_t)call >= ctx->reproPeaks.size() || (cap && !out)) return GX_ERR_ORDER;
  const size_t n = std::min(cap, ctx->reproPeaks[call].size());
  if (n) memcpy(out, ctx->reproPeaks[call].data(), n * sizeof(gx_peak));
  return GX_OK;
}

int gx_write_reproducibility(gx_ctx* ctx, int pct, FILE* calls_file, FILE* metrics_file) {
  if (!ctx || (!calls_file && !metrics_file) || ctx->reproCalls.empty() || !ctx->peaksReady || pct < 0 || pct > 100) return GX_ERR_ORDER;
  const size_t nC = ctx->reproCalls.size();
  const int nR = (int)((nC - 2) / 3);
  const gx_peak* run = static_cast<const gx_peak*>(ctx->hPeaks.p);
  std::vector<const gx_peak*> lists(nC);
  for (size_t i = 0; i < nC; i++) lists[i] = ctx->reproPeaks[i].data();
  gx_repro_figures fig;
  std::vector<uint64_t> pairs((size_t)nR * (nR - 1) / 2 + 1), self((size_t)nR), inRun(nC), runSup(nC);
  if (int rc = gx_reproducibility_figures(run, ctx->nHostPeaks, nR, ctx->reproCalls.data(), lists.data(), pct, &fig, pairs.data(), self.data(),
                                          inRun.data(), runSup.data(), nullptr, nullptr))
    return rc;
  if (calls_file)
    if (int rc = gx_format_reproducibility(calls_file, nR, ctx->reproCalls.data(), inRun.data(), runSup.data(), ctx->nHostPeaks, ctx->peakBP, pct,
                                           ctx->reproSeed))
      return rc;
  if (metrics_file)
    if (int rc = gx_format_reproducibility_metrics(metrics_file, &fig, pairs.data(), self.data())) return rc;
  return GX_OK;
}

int gx_set_phase_timing(gx_ctx* ctx, int level) {
  if (!ctx || level < 0 || level > 2) return GX_ERR_ORDER;
  ctx->phaseLevel = level;
  return GX_OK;
}

int gx_phase_times(gx_ctx* ctx, const char** names, const float** ms) {
  if (!ctx) return 0;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  ctx->phaseMs.clear();
  ctx->phaseNames.clear();
  for (size_t i = 0; i < ctx->nPhases; i++) {
    Phase& ph = ctx->phases[i];
    float t = 0;
    (void)hipEventElapsedTime(&t, ph.a, ph.b);
    ctx->phaseMs.push_back(t);
    ctx->phaseNames += ph.name;
    ctx->phaseNames.push_back('\0');
  }
  if (names) *names = ctx->phaseNames.c_str();
  if (ms) *ms = ctx->phaseMs.data();
  return (int)ctx->nPhases;
}

}  // extern "C"
