// gx_host_ctx.h -- the context behind the C ABI: device / pinned buffers, the per-run records, the test switches, the mail
// block and the re-evaluation of risky p-values (gx_math.h round_checked).
// (a part of gx_api.hip's translation unit: the kernels are templates and inline functions of the headers it includes;
// split by phase -- context / build / stats / sweep / collectives -- in round 5)
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <string>
#include <vector>
#include <unistd.h>

#include "gx_merge.h"
#include "gx_rccl.h"
#include "gx_sort.h"
#include "gx_tile_fast.h"
#include "gx_sbtile.h"
#include "gx_dups.h"
#include "gx_bhx.h"
#include "gx_saturate.h"
#include "gx_count.h"
#include "gx_regions.h"
#include "gx_coverage.h"
#include "gx_profile.h"
#include "gx_gram.h"
#include "gx_fingerprint.h"
#include "gx_rank.h"
#include "gx_complexity.h"
#include "gx_ivstat.h"
#include "gx_xcor.h"
#include "gx_gcbias.h"
#include "gx_motifs.h"
#include "gx_kmers.h"
#include "gx_subsample.h"
#include "gx_depth.h"
#include "gx_peaksig.h"
#include "gx_summits.h"

using namespace gx;

namespace {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), own(o.own) { o.p = nullptr; o.cap = 0; o.own = true; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; own = o.own; o.p = nullptr; o.cap = 0; o.own = true; }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p && own) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    own = true;
  }
  void view(void* ptr, size_t bytes) {  // non-owning window into another allocation
    release();
    p = ptr;
    cap = bytes;
    own = false;
  }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
  bool own = true;
};

// Small device -> host read-backs land in one pinned block: a copy into pageable memory is staged and
// blocks the caller, a copy into pinned memory is an ordinary asynchronous packet.
struct HostMail {
  Scalars scal;
  long long acc[2];
  uint64_t peakBP, genome;
  u32 nF, nIv, status, R, nPeaks, nMerged, D, n, hot, bhOvf;
  long long coll[4];   // this rank's / all ranks' {fragLen parts, saturation flag}
  u32 counts[64];      // BH records per rank (all-gather)
  u32 closeState;      // k_scan_iv_close: 1 the sample is closed, 2 the separate kernels have to run
  u32 statusKeep;      // (host -> device: the status bits a repeated tile stage must keep)
  u32 seq;             // k_mail's last write (mail_sync polls it)
};

struct PinnedBuf {
  void* p = nullptr;
  void* dp = nullptr;  // the same memory as the device sees it (kernels write results straight into it)
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 4 + 4096;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocMapped | hipHostMallocCoherent);  // (fine-grained: the kernels write mail and peaks into it while the host polls)
    if (e == hipSuccess) {
      cap = want;
      e = hipHostGetDevicePointer(&dp, p, 0);
    }
    return e;
  }
};

struct Pileup {  // run-length pileup of one sample (treatment or control)
  DevBuf ivEnd, ivV, tileIvOff, chromIvOff;
  u32 nIv = 0;
  bool packed = false;  // ivEnd / ivV filled (otherwise the intervals still sit in the loose slots)
  // a sample that waits for its control merge where the tile stage left it (stash_loose): its loose slots and its tile
  // descriptors (slot, carry) taken out of the context, which builds the next sample into other buffers
  DevBuf looseEnd, looseV, meta;
  bool inLoose = false;
};

struct PArray {  // p-value intervals of one replicate (or the Fisher combination)
  DevBuf end, p, expt, ctrl, chromOff, tileOff, q, dPresent;
  u32 n = 0;
  bool loose = false;     // no control: the intervals still sit in the tile kernel's loose slots (ctx->looseEnd / looseV);
                          // the tight table is made when somebody asks for it (materialize_rep)
  bool looseSweep = false;    // ... and the tile stage left the sweep's significance bits for them (LooseCtl): gx_find_peaks on
                              // this replicate alone, with -p, walks the loose slots as they are
  DevBuf chromLooseOff;       // [nChrom + 1] first loose slot of each chromosome
  size_t looseStride = 0;     // words between the sig / brk masks in swMask
  bool pilesPending = false;  // the pileup floats are wanted but not made yet (ensure_piles)
  bool pairPending = false;   // ... with a control: to be made from the merge's loose arrays, the two samples' tile offsets and the
                              // control's tables, which all last until the next sample begins (make_pair_piles)
  bool mergedP = false;       // ... by a merge that wrote p-values, not pileups, into its loose slots (k_merge2<.., true>): the
                              // pileups' merge runs when the floats are asked for
  // ... and what they will be made from once the context has built another sample into its loose slots: this replicate's
  // exact pileups and tile descriptors, taken out of the context (no copy; the context takes other buffers: pooled)
  DevBuf keptV, keptMeta;
  bool keptLoose = false;
  bool latePending = false, lateLoose = false;   // the loose sweep's bits are still to be written (k_loose_late) / were written late
  bool qLazy = false;     // -q: q[] holds the candidates' intervals only; the rest on request (ensure_q)
  bool hasPiles = false;  // expt/ctrl filled (single-replicate logging)
  bool pilesDropped = false;  // ... deliberately not (gx_set_keep_pileups(0))
  float ctrlConst = 0.0f; // control value when ctrl is not materialised (no -E, no control file)
  bool ctrlIsConst = false;
  std::vector<uint8_t> present;  // per chromosome: p-values exist (pval[n] != NULL)
};

struct Phase {
  std::string name;
  hipEvent_t a, b;
};

// Test and measurement switches.  They are read from the environment ONCE, when the context is made (gx_create), or
// set on a live context by gx_set_knob; nothing in a build or a sweep calls getenv.  Every one of them is exercised
// by tests/ (a forced path must give the oracle's bits like the default one) or by tools/.
struct Knobs {
  int debug = 0;          // GX_DEBUG: synchronise after every launch and say which kernel it was
  int debugRetry = 0;     // GX_DEBUG_RETRY: say why a sample was built again
  int noSpin = 0;         // GX_NO_SPIN: block in the runtime instead of polling for the mail
  int forceRec64 = 0;     // GX_FORCE_REC64: 8-byte records although the genome fits 4-byte keys (only > 4.29 Gbp takes them naturally)
  int forceSlowFrag = 0;  // GX_FORCE_SLOWFRAG: the general fragLen path
  int noFused = 0;        // GX_NO_FUSED: the general chain instead of k_sbtile
  int noLoose = 0;        // GX_NO_LOOSE: lambda after the tile stage, tight table, the sweep on it
  int noPairs = 0;        // GX_NO_PAIRS: k_sort1's start / end keys for k_sbtile
  int noFracPairs = 0;    // GX_NO_FRAC_PAIRS: fractional weights take the general chain
  int noBedFused = 0;     // GX_NO_BED_FUSED: a run with -E regions takes the general chain (k_tile<BED>), as until round 5
  int bhVariant = -1;     // GX_BH_VARIANT: the instance of k_bh_hist / k_qlookup (0: 256 threads, 2048-entry LDS tables -- rounds 2-5; 1: 1024 threads,
                          // one workgroup per CU, 8192 / 16384 entries; 2: 512 threads, 4096 / 8192 entries); default: chosen by the run
  int mergeWg = 0;        // GX_MERGE_WG: the control merge by k_merge2 (a workgroup per tile, rounds 2-5) instead of k_merge2w (a wavefront per tile)
  int noQLoose = 0;       // GX_NO_Q_LOOSE: -q on one replicate without control makes the tight table and sweeps it, as until round 6
  int noLateLoose = 0;    // GX_NO_LATE_LOOSE: a sample whose lambda comes with its end takes the tight table (k_pack_pval), as until round 6
  int noLazyQ = 0;        // GX_NO_LAZY_Q: q of every interval by k_qlookup, as until round 6
  int noPackHist = 0;     // GX_NO_PACK_HIST: BH's histogram by k_bh_hist from the tight table also for a single replicate without control
  int noMergeP = 0;       // GX_NO_MERGE_P: the control merge leaves both pileups in its loose slots and k_pack_pairs scores them, as until round 5
  int forceHalfBins = 0;  // GX_FORCE_HALF_BINS: the 128-key level 1 on a small input
  int noHalfBins = 0;     // GX_NO_HALF_BINS
  int fracHalfBins = 0;   // GX_FRAC_HALF_BINS: half-size bins also for a dense sample with fractional weights (measurements)
  int noEarlyColl = 0;    // GX_NO_EARLY_COLL: no all-reduce of the closed form of fragLen ahead of the tile stage
  int regWindows = 0;     // GX_REG_WINDOWS: gx_count_in_regions keeps its histograms in LDS up to this many windows (default REG_WIN_MAX; < 0: never)
  int noDenseBh = 0;      // GX_NO_DENSE_BH: the range-partitioned exchange also without a control
  int qtMulti = 0;        // GX_QT_MULTI: the chunked BH table kernels for a small table
  int forceColl = 0;      // GX_FORCE_COLL: run the collectives with a single rank too
  int sbShift = -1;       // GX_SBSHIFT: tiles per super-bucket (log2)
  long long runCapMin = 0;  // GX_RUN_CAP_MIN: the sweep's first guess of the run count (a tiny one forces the second pass)
  int bhCapLog = 0;       // GX_BH_CAPLOG: log2 of the BH table's first size
  int ptJmax = 0;         // GX_PT_JMAX: pages per level-1 list at first
  int sbtTr = 0;          // GX_SBT_TR: 384 / 448: which instance of k_sbtile's dense launch runs (measurements; default: by the sample's density)
  int sbtGrid = 0;        // GX_SBT_GRID: persistent workgroups of k_sbtile's first launch (0: one per CU; a small number makes one workgroup run
                          // many bins in a row: tests, measurements)
  int sweepGrid = 0;      // GX_SWEEP_GRID: persistent workgroups of the sweep's look-back kernels and of either half of k_scan_iv_close_runs
                          // (0: as many as are resident together; tests: 1 makes one workgroup walk every chunk)
  int noSweepOverlap = 0; // GX_NO_SWEEP_OVERLAP: the sweep's run pass behind the sample's closing (k_runs), as until round 25
  int s2Grid = 0;         // GX_S2_GRID: persistent workgroups of k_sort_a (per piece) and k_sort_b (0: as many as are resident together; a small
                          // number makes one workgroup run many chunks / pages in a row: tests, measurements)
  int fpAgg = 0;          // GX_FP_AGG: k_fp_hist aggregates equal classes inside the wavefront before LDS (measurements; default: an atomic pair per lane)
  int rankCapLog = 0;     // GX_RANK_CAP_LOG: log2 of the first capacity of k_rank_distinct's table (default RK_CAP_LOG; tests: the growth path with a few thousand values)
  int rankLookup = 0;     // GX_RANK_LOOKUP: k_rank's lookup: 1 binary search in the sorted table, 2 probing a hashed one (measurements; default RK_LOOKUP)
  int depthGrid = 0;      // GX_DEPTH_GRID: workgroups of k_depth_hist (0: one per DEPTH_NW tiles, at most DEPTH_GRID; tests: 1 makes one workgroup walk every tile)
  int depthListCap = 0;   // GX_DEPTH_LIST_CAP: entries of k_depth_hist's deep list at first (0: DEPTH_LIST_CAP; tests: a tiny one forces the rerun)
  int depthPriv = 0;      // GX_DEPTH_PRIV: k_depth_hist<true> sums the pieces of whole depth 1 .. 4 in registers, one LDS atomic per class and wavefront (measurements; default: an LDS atomic per piece)
  int xcorGrid = 0;       // GX_XCOR_GRID: workgroups of k_xc_corr at gx_sample_end (0: one per tile, at most XC_GRID; tests: 1 makes one workgroup walk every tile)
  int xcorTile = 0;       // GX_XCOR_TILE: plus words per tile of k_xc_corr at gx_sample_end (0: XC_TILE; tests: 64 puts many tile borders into a small genome)
  int roctx = 0;          // GX_ROCTX: a roctx range around every phase (rocprofv3 --marker-trace: kernel -> phase attribution)
  int fault = 0;          // GX_FAULT: fault injection for the tests of the device-side invariants.  1: the weight of the ends at
                          // chromosome 0's length is damaged behind level 1 of the sort (as if an end record had been lost)
};
// Every decision of one build of a sample, made once (plan_build, gx_host_build.h) before anything is sized, cleared or
// launched; the stages read it and nothing else decides.  The context keeps the last one (`built`): finish_scalars, the
// retries, gx_pvalues and gx_path_info ask it what ran.
struct BuildPlan {
  int isCtrl = 0;
  bool reuseSort = false;   // only the tile stage runs again, on the general chain, over level 1's pages (close_sample)
  u32 nEv = 0;
  bool unit32 = false;      // tile id + offset fit a 4-byte key
  bool multiRank = false;
  bool earlyColl = false;   // the ranks exchange the closed form of fragLen ahead of the tile stage
  bool fused = false;       // the tile stage is k_sbtile
  bool pairs = false;       // ... on level 1's pair records (k_sort_a / k_sort_b)
  bool fracPairs = false;   // ... with a weight class per record (fractional weights)
  int sbS = 0;              // log2 of the tiles per level-1 bin (the context's, or one less: half-size bins)
  u32 nL1 = 0;              // level-1 bins
  u32 nCoarse = 0, jmaxC = 0, nWG1 = 0;   // pair mode's first pass: coarse lists, pages per list, its workgroups over all pieces
  u32 jmax = 0;             // pages per (XCD class, bin) list
  u32 poolPages[3] = {0, 0, 0};
  bool wantEarly = false;   // lambda ahead of the tile stage: it writes the sweep's bits on the loose slots
  bool wantLate = false;    // ... after the table p(V) (k_loose_late)
  bool closeInScan = false; // the scan's last workgroup closes the sample (k_scan_iv_close)
  bool dense = false;       // k_sbtile: one launch takes every bin by rounds
  bool denseSmall = false;  // ... in the instance with the smaller scratch (SBT_TR_DENSE)
  bool fragFused = false;   // the tile kernel adds the general fragLen path's terms itself (TileIn::fragAcc)
  size_t looseCap = 0, ivCap = 0;
  u32 tChunks = 0;
  bool masks() const { return wantEarly || wantLate; }   // the sweep's masks are the loose slots'
};
// Every decision of one gx_find_peaks, made once (plan_call, gx_host_call.h) before anything is sized, cleared or launched;
// the stages read it and nothing else decides.  The context keeps the last one (`called`), with what only the run could
// tell (`ran`): gx_path_info reports the calling half's bits from it.
struct CallPlan {
  enum Walk { TIGHT, LOOSE_P, LOOSE_Q };             // what the sweep walks: the final array's tight table, or the loose slots
  enum Bh { BH_NONE, BH_SMALL, BH_FROM_DENSE, BH_FROM_HIST };   // BH's table: none (-p); loose_hist + k_bh_small; from the "bp at V"
                                                     // sums k_pack_pval<.., HIST> left; by k_bh_hist from the tight table
  enum Exchange { X_NONE, X_DENSE, X_RANGE };        // the ranks' exchange of that table, as intended (X_DENSE may fall back: ran)
  enum Masks { MASKS_TILE, MASKS_PACK, MASKS_BH, MASKS_SIG };   // who fills the sweep's masks: the tile stage (/ k_loose_late), the
                                                     // pack kernel that wrote the tight table, BH, or the sweep's own k_sig_mask
  Walk walk = TIGHT;
  bool lateWrite = false;   // the loose slots' bits are still to be written (k_loose_late; LOOSE_Q: from "q passes from this pileup on")
  bool lateBefore = false;  // ... were written behind the tile stage by a call before this one
  bool packHist = false;    // the tight table's kernel sums BH's histogram on its way (k_pack_pval<.., HIST>)
  u64 materialise = 0;      // reps[] entries (a bit each) whose tight table is made now
  bool keepLoose = false;   // those whose pileup floats are pending keep what they are made of: the loose slots are about to be reused
  bool combine = false;     // Fisher's method over the replicates (combine_replicates)
  int finalIdx = -1;        // reps[] entry the peaks are called on
  bool genomeOpt = false;   // the genome length is computed (no -L): BH's lengths must add up to it
  u64 g = 0;
  bool setMisc = false;     // k_set_misc: genome length and interval count for the kernels that read them through pointers
  Bh bh = BH_NONE;
  Exchange exchange = X_NONE;
  int bhInst = 0;           // row of BH_INSTANCES (GX_BH_VARIANT, or the default)
  bool lazyQ = false;       // q inside the candidates only (k_sig_from_p / k_q_fill_cands), the whole array on request
  bool qtMulti = false;     // the chunked q-table kernels whatever the table's size (GX_QT_MULTI)
  Masks masks = MASKS_SIG;
  bool specOk = false;      // the run pass that rode in the scan's launch saw the very bits this sweep walks
  bool qLooseBad = false;   // the second plan of a call: LOOSE_Q was called off (ST_Q_LOOSE)
  struct Ran {
    bool denseFellBack = false;  // a rank's region of the dense exchange overflowed: the range exchange ran instead
    bool tableGrew = false;      // BH's table was full (ST_HASH_FULL) and made again, larger, by k_bh_hist
    bool overlap = false;        // the sweep took the speculative run pass
    bool lateWritten = false;    // k_loose_late ran
  } ran;
  bool looseSwept() const { return walk != TIGHT; }
  bool lateBits() const { return lateBefore || ran.lateWritten; }
};
struct KnobDef { const char* name; int Knobs::*i; long long Knobs::*ll; };
const KnobDef KNOBS[] = {
    {"GX_DEBUG", &Knobs::debug, nullptr}, {"GX_DEBUG_RETRY", &Knobs::debugRetry, nullptr}, {"GX_NO_SPIN", &Knobs::noSpin, nullptr},
    {"GX_FORCE_REC64", &Knobs::forceRec64, nullptr}, {"GX_FORCE_SLOWFRAG", &Knobs::forceSlowFrag, nullptr},
    {"GX_NO_FUSED", &Knobs::noFused, nullptr}, {"GX_NO_LOOSE", &Knobs::noLoose, nullptr}, {"GX_NO_PAIRS", &Knobs::noPairs, nullptr},
    {"GX_NO_FRAC_PAIRS", &Knobs::noFracPairs, nullptr}, {"GX_NO_BED_FUSED", &Knobs::noBedFused, nullptr}, {"GX_NO_MERGE_P", &Knobs::noMergeP, nullptr}, {"GX_NO_PACK_HIST", &Knobs::noPackHist, nullptr}, {"GX_NO_LAZY_Q", &Knobs::noLazyQ, nullptr}, {"GX_NO_LATE_LOOSE", &Knobs::noLateLoose, nullptr}, {"GX_NO_Q_LOOSE", &Knobs::noQLoose, nullptr}, {"GX_MERGE_WG", &Knobs::mergeWg, nullptr}, {"GX_BH_VARIANT", &Knobs::bhVariant, nullptr}, {"GX_FORCE_HALF_BINS", &Knobs::forceHalfBins, nullptr},
    {"GX_NO_HALF_BINS", &Knobs::noHalfBins, nullptr}, {"GX_FRAC_HALF_BINS", &Knobs::fracHalfBins, nullptr}, {"GX_NO_EARLY_COLL", &Knobs::noEarlyColl, nullptr},
    {"GX_NO_DENSE_BH", &Knobs::noDenseBh, nullptr}, {"GX_REG_WINDOWS", &Knobs::regWindows, nullptr}, {"GX_QT_MULTI", &Knobs::qtMulti, nullptr}, {"GX_FORCE_COLL", &Knobs::forceColl, nullptr},
    {"GX_SBSHIFT", &Knobs::sbShift, nullptr}, {"GX_RUN_CAP_MIN", nullptr, &Knobs::runCapMin}, {"GX_BH_CAPLOG", &Knobs::bhCapLog, nullptr},
    {"GX_PT_JMAX", &Knobs::ptJmax, nullptr}, {"GX_FAULT", &Knobs::fault, nullptr}, {"GX_SBT_TR", &Knobs::sbtTr, nullptr}, {"GX_SBT_GRID", &Knobs::sbtGrid, nullptr},
    {"GX_S2_GRID", &Knobs::s2Grid, nullptr}, {"GX_SWEEP_GRID", &Knobs::sweepGrid, nullptr}, {"GX_NO_SWEEP_OVERLAP", &Knobs::noSweepOverlap, nullptr},
    {"GX_FP_AGG", &Knobs::fpAgg, nullptr},
    {"GX_RANK_CAP_LOG", &Knobs::rankCapLog, nullptr},
    {"GX_RANK_LOOKUP", &Knobs::rankLookup, nullptr},
    {"GX_DEPTH_GRID", &Knobs::depthGrid, nullptr}, {"GX_DEPTH_LIST_CAP", &Knobs::depthListCap, nullptr}, {"GX_DEPTH_PRIV", &Knobs::depthPriv, nullptr},
    {"GX_XCOR_GRID", &Knobs::xcorGrid, nullptr}, {"GX_XCOR_TILE", &Knobs::xcorTile, nullptr},
    {"GX_ROCTX", &Knobs::roctx, nullptr},
};
// a switch that is merely present counts as 1 (GX_NO_LOOSE= is "on", as it was with getenv() != nullptr), and so does a
// value that is not a number (GX_NO_LOOSE=yes)
bool set_knob(Knobs& k, const char* name, const char* value) {
  for (const KnobDef& d : KNOBS)
    if (!strcmp(d.name, name)) {
      long long v = 1;
      if (value && *value) {
        char* end = nullptr;
        v = strtoll(value, &end, 10);
        if (end == value) v = 1;
      }
      if (d.i) k.*(d.i) = (int)v; else k.*(d.ll) = v;
      return true;
    }
  return false;
}

}  // namespace

struct gx_ctx {
  gx_params par{};
  Knobs knob;
  int device = 0;
  hipStream_t stream = nullptr;
  bool keepPiles = true;        // materialise the pileup floats of the p-value intervals
  int maskIdx = -1;             // reps[] entry whose sig / skip masks sit in swMask (k_pack_pval)
  u32 maskN = 0;
  size_t maskStride = 0;        // words between the sig / skip / brk masks in swMask
  hipStream_t side = nullptr;   // small read-backs that must not stall the main stream
  hipEvent_t sideEv = nullptr;
  std::string err;
  // chromosome table
  std::vector<uint32_t> len;
  std::vector<uint8_t> skip, save, owned;
  std::vector<std::vector<uint32_t>> bed;
  std::vector<DChrom> hChrom;
  u32 nChrom = 0, nTiles = 0;
  int sbShift = 0;
  u32 nSB = 0;
  DevBuf dChrom, dTileChrom, dBedTileOff, dBedEdge, dTileSave0;
  bool hasBed = false;
  bool bedGiven = false;        // some chromosome (of any rank) has -E regions: what every rank knows alike
  size_t nBedEdges = 0;
  // per-sample state
  int phase = 0;  // 0 idle, 1 treatment open, 2 treatment done, 3 control open, 4 control done
  int sample = 0;
  // The sample's events, in push order: device-resident segments of the caller (gx_push_events_device) and
  // pieces of the library's own device chunks, filled from host memory by asynchronous copies on `side`
  // (`ready` = the copy has arrived: the main stream waits for it before the kernel that reads the piece).
  struct Seg { const gx_event* p; size_t n; hipEvent_t ready; bool packed = false; };   // (packed: 8-byte gx_event8 records behind p)
  std::vector<DevBuf> unpackBufs; // packed pieces as 16-byte events, for the paths that read those (unpack_segs); reused sample after sample
  size_t unpackUsed = 0;
  std::vector<Seg> segs;
  std::vector<DevBuf> evChunks;   // device chunks of EV_CHUNK events, reused sample after sample
  size_t evChunkIdx = 0, evChunkFill = 0;
  PinnedBuf stage[2];             // pinned staging of gx_push_events (the caller's buffer is free on return)
  hipEvent_t stageFree[2] = {nullptr, nullptr};
  int stageNext = 0;
  std::vector<hipEvent_t> evPool; // `ready` events, reused
  size_t evPoolUsed = 0;
  DevBuf satBuf;                  // what gx_filter_saturation left of the sample
  struct Stream {  // one record stream of the bucket sort
    DevBuf a, pool, pt, cursor, sbOff;  // level-2 output; level-1 pages, page table, list cursors; super-bucket offsets
  };
  size_t b2LdsSet = 0;          // dynamic LDS the level-2 kernel was last configured for
  bool sbtLdsSet = false;       // ... and k_sbtile
  bool sawFrac = false;         // a sample of this context HELD fractional weights (learned: ST_SB_FRAC, Scalars::fracSeen): no closed
                                // form of fragLen, no early lambda, no loose-slot sweep from then on
  bool fracHint = false;        // gx_expect_fractional: only selects the kernels that can carry a weight class (k_sort_a<true>,
                                // k_sbtile<.., true>); on unit-weight data they give what the unit-weight instances give
  bool fusedOff = false;        // this sample: a super-bucket did not fit k_sbtile (the general chain runs instead)
  BuildPlan built;              // the last build's plan
  CallPlan called;              // the last gx_find_peaks' plan, and what its run told
  bool earlyOwed = false;       // built.earlyColl, and this rank has not taken part in that all-reduce yet (poison_allreduce)
  bool earlyPending = false;
  int fusedBackoff[2] = {0, 0}; // treatment / control samples for which k_sbtile is not tried (after one that did not fit)
  bool pilesMade = false;       // pileup floats were written since the last gx_reset (ensure_piles)
  bool mergePUsed = false;      // the last control merge wrote p-values into its loose slots (k_merge2<.., true>)
  DevBuf lbSweep, lbSweep2;     // look-back granules of the sweep's one-pass compactions (generation-tagged)
  u32 sweepGen = 0;
  FragSelect closeSel{};        // the sample's k_frag_select arguments (k_scan_iv_close took them; finish_scalars may need them again)
  u32 closeSeq = 0;             // sequence number of the mail k_scan_iv_close sends (0: the separate kernels were launched)
  bool beginPending = false;    // gx_sample_begin's clearing of the scalars is still to be done (k_build_init / flush_begin)
  u64 beginGenome = 0;
  bool fellBack = false;        // some sample was sent back from k_sbtile to the general chain
  bool ptGrew = false;          // some sample was built again with larger page tables (RETRY_PT)
  bool packedUsed = false;      // the last build read a piece of 8-byte events in place (k_sort_a<.., PACKED>: gx_path_info)
  bool looseOk = false;         // the treatment sample's tile stage left valid sweep bits on the loose slots
  bool riskNearThr = false;     // a re-evaluated table entry lies next to the significance threshold
  size_t looseStride = 0;       // words between the sig / brk masks the tile stage wrote into swMask
  DevBuf tileSlot, chromW0, chromLooseOff, looseCtl;
  u32 ptJmax = 16;              // pages per (XCD class, super-bucket) list; grown after ST_PT_FULL
  DevBuf lbIv;
  Stream str[3];  // S (start keys), E (end keys), F (fractional records)
  DevBuf tileCnt[3], tileOff[3];
  DevBuf looseC, looseC2, pairLogE, pairCtab, pairP2d, fragSum, tileDeep, fragList, zeroArena, endAtLen, binNet, curC, ptC, poolC, auxC, nWide, wideList, heavyList;
  size_t arenaBytes = 0;        // what the views into zeroArena cover: one launch clears it (k_build_init)
  DevBuf tileMeta, tileWsum, tileCarry, lb, misc, dScal, dStatus, looseEnd, looseV, tileIvCount, tileLastEnd, tilePrevEnd;
  Pileup expt, ctrl;
  Scalars hScal{};  // host copy of the device scalars (refreshed from the mail block)
  std::vector<PArray> reps;
  int finalIdx = -1;
  // BH
  DevBuf pvLut, dRisk, dDeep;
  PinnedBuf riskHost;           // count + records of the risky p-values, as read back / as sent with the host's values
  bool pairTabsReady = false;   // the control's p-value tables were built when its sample was closed
  DevBuf bhKeys, bhLens, bhOutKeys, bhOutSlot, bhSortKeys, bhSortSlot, bhQ, bhKQ, bhRaw, bhDl, bhTmp, bhRecs;
  PinnedBuf hostRecs;           // this rank's BH records for the all-gather
  bool satDone = false;         // this sample's events already went through the saturation filter
  long long satDropped = 0;     // ... which dropped this many of them (gx_saturation_dropped)
  bool qLooseBad = false;       // -q on the loose slots was called off once (ST_Q_LOOSE): this context takes the tight table from now on
  DevBuf qLut;                  // -q on the loose slots: q by whole pileup (k_bh_small)
  bool bhLive = false;          // the table of the last -q run is still there, with {key, q} of every value (lazy q: ensure_q)
  u32 bhLiveCap = 0;
  int bhLiveIdx = -1;           // ... and it belongs to reps[bhLiveIdx]
  bool bhDirty = false;         // the BH table was left with entries (an error path): wipe it before use
  u32 bhCapLog = 22;            // log2 of its slots (grows by 3 after ST_HASH_FULL)
  // sweep
  DevBuf swStart, swEnd, swMask, cand, valid, peaks, headPos, candHdr, longList;
  PinnedBuf hPeaks;             // the peak list on the host (pinned: the read-back is asynchronous)
  size_t nHostPeaks = 0;
  u32* nIvTarget = nullptr;
  PinnedBuf mailBuf;
  HostMail* mail = nullptr;
  uint64_t genomeLenUsed = 0, peakBP = 0;
  // collectives
  int rank = 0, world = 1;
  gx_allreduce_i64_fn allreduce = nullptr;
  void* user = nullptr;
  ncclComm_t comm = nullptr;    // the library's own collectives (gx_set_rccl): RCCL on device buffers, on `stream`
  bool forceColl = false;       // GX_FORCE_COLL=1: run the collectives with a single rank too (tests)
  DevBuf bigBins;               // pair mode: the super-buckets k_sbtile's first launch leaves to its second
  DevBuf dColl, dCounts, dGather, bhDense, bhxSmall, bhxRecv, bhxKeys, bhxLens, bhxQ, bhxOut, bhxAns;
  int phaseLevel = 0;       // gx_set_phase_timing
  std::string phaseFilter = "tile";  // level 1: the one phase that is timed (gx_set_phase_filter)
  u32 mailSeq = 0;          // mail_sync: the sequence number the next k_mail writes
  u32 statusSeen = 1;       // status bits read back since the device word was last cleared (1: not cleared yet)
  u64 runCap = 0, runSeen = 0;  // run_sweep: runs its arrays are sized for; runs of the last sweep
  // the sweep's run pass launched ahead of time, in the scan's launch (k_scan_iv_close_runs: spec_runs); run_sweep's first
  // attempt takes it when the sweep turns out to be the one it was launched for, and drops it in every other case
  struct SpecRuns {
    bool valid = false;
    u32 gen = 0, cap = 0, nWords = 0;   // its generation number, the run arrays' capacity, the mask's words ...
    size_t stride = 0;                  // ... and the words between the masks
  } specRuns;
  int buildAttempt = 0;         // close_sample: builds of the sample before this one (a rebuilt sample speculates nothing)
  int resScanRuns = 0;          // co-resident workgroups of k_scan_iv_close_runs
  bool phaseOpen = false;
  bool roctxOpen = false;       // (GX_ROCTX: the range of the open phase)
  int numCU = 0, resTile = 0, resTileHalf = 0, resTileFast = 0, resSweep = 0;  // co-resident workgroups per kernel class
  int resSortA = 0, resSortB = 0;   // ... of k_sort_a (the fewest of its four instances: one grid rule for every piece) and k_sort_b
  // recycled device buffers (gx_reset keeps allocations alive across runs)
  std::vector<DevBuf> pool;
  // counting in peaks (gx_set_count_in_peaks / gx_count_in_peaks, gx_count.h): every closed sample's events stay where they are
  struct KeptSample {
    int rep = 0;
    bool ctrl = false;
    std::vector<Seg> segs;          // as gx_sample_end left them (after the int16 rule: the survivors in `sat`)
    std::vector<uint8_t> save;      // the chromosomes its pileup took (Chrom.save of its replicate's treatment file)
    std::vector<DevBuf> chunks, unpacks;  // the library's buffers behind `segs`, taken out of evChunks / unpackBufs
    DevBuf sat;
  };
  bool countOn = false;
  bool peaksReady = false;        // gx_find_peaks has called the peaks of the samples kept so far
  bool countsReady = false;       // ... and gx_count_in_peaks has counted them
  std::vector<KeptSample> kept;
  // what a pass over kept events reads besides them (gx_host_kept.h kept_stage): its staging area and the device's copy.  One
  // pair serves all the passes: each drains the stream before it returns.  Likewise the one copy of a caller's events that the
  // *_events hooks read (kept_upload).
  PinnedBuf keptStage;
  DevBuf keptIn;
  DevBuf hookEv;
  u32 cntPk = 0;                  // peaks of the last count
  DevBuf cntIdx, cntDiff, cntRes;
  PinnedBuf cntHost;
  bool cntLdsSet = false;
  // counting in regions (gx_count_in_regions, gx_regions.h): the same kept samples, result buffers of its own
  bool regionsReady = false;      // gx_count_in_regions has counted: regSamples samples in regN regions
  size_t regN = 0;
  u32 regSamples = 0;
  u32 regInvCap = 1u << 14;       // REG_INV_CAP, or more after a pass that met more inverted intervals
  DevBuf regIdx, regHist, regSums, regRes, regInv;
  PinnedBuf regHost;
  bool regLdsSet = false;
  // binned coverage (gx_set_coverage_bins, gx_coverage.h): every closed sample's pileup summed over bins of covW bases
  struct CovSample {
    int rep = 0;
    bool ctrl = false;
    DevBuf bins;                  // int64 per bin, chromosome c's from covOff[c] on
  };
  u32 covW = 0;                   // 0: off
  bool covDirty = true;           // the chromosome table changed since covOff was laid out
  std::vector<size_t> covOff;     // [nChrom + 1] first bin of each chromosome (one without bins here: as many as the next)
  DevBuf covChromBin;             // ... for the device (u32)
  std::vector<CovSample> cov;     // until gx_reset
  // profiles around anchors (gx_set_profile, gx_profile.h): every closed sample's pileup summed over windows around them
  struct ProfSample {
    int rep = 0;
    bool ctrl = false;
    DevBuf agg;                   // int64 per bin
    DevBuf cells;                 // int64 per anchor and bin, in the caller's anchor order (profKeep)
  };
  std::vector<gx_anchor> profAnchors;   // empty: off
  u32 profF = 0, profB = 0, profNb = 0;
  bool profKeep = false;
  bool profDirty = true;          // the chromosome table changed since profDev was made
  DevBuf profDev;                 // ProfAnchor per anchor
  DevBuf profPartial;             // k_profile's workgroups' sums
  std::vector<ProfSample> prof;   // until gx_reset
  // the statistics over the bins (gx_host_binstat.h) share two buffers; nothing here exists before the first call.  Sharing is
  // safe because every pass that uses them drains the stream before it returns (each reads its results back): no pass is in
  // flight when the next one stages rows or uploads pointers.
  DevBuf statRows;                // the row pointers for the device: the 32 rows read, then the 32 rows written
  DevBuf statIn;                  // the *_u64 hooks' copy of the caller's rows
  // the samples' Gram sums (gx_coverage_gram / gx_gram_u64, gx_gram.h)
  DevBuf gramPartial, gramOut;    // k_gram's workgroups' sums, k_gram_sum's totals
  bool gramUsed = false;          // the kernels ran since the last gx_reset
  // the samples' fingerprint histograms (gx_coverage_fingerprint / gx_fp_u64, gx_fingerprint.h)
  DevBuf fpOut;                   // count[S][FP_NC], sum[S][FP_NC]
  bool fpUsed = false;            // the kernel ran since the last gx_reset
  // the samples' rank rows (gx_coverage_distinct / gx_coverage_rank_gram / gx_distinct_u64 / gx_rank_u64, gx_rank.h)
  DevBuf rankTab, rankCtl;        // k_rank_distinct's table (keys, then counts) and the control words (RKC_*)
  DevBuf rankPairs;               // k_rank_compact's (value, count) pairs
  DevBuf rankLut;                 // k_rank's tables: the samples' values, their rank2, the offsets
  DevBuf rankOut;                 // the rank rows k_gram reads
  bool rankUsed = false;          // k_rank ran since the last gx_reset
  u32 rankLastCapLog = 0, rankLastGrown = 0;   // the last k_rank_distinct pass: log2 of the capacity it ended with, how often it grew (gx_rank_last)
  // library complexity of the kept samples' intervals (gx_complexity / gx_complexity_events, gx_complexity.h); nothing here
  // exists before the first call
  struct CpxResult {
    int rep = 0;
    bool ctrl = false;
    u64 N = 0, D = 0;               // observations, distinct keys
    std::vector<uint64_t> mult, keys;   // h, sparse: keys[i] keys were seen mult[i] times (mult ascending)
  };
  DevBuf cpxTab, cpxCtl, cpxBig;  // the table (reused sample after sample), the control words + k_cpx_hist's histogram, its list
  std::vector<CpxResult> cpx;     // the last gx_complexity, per kept sample (until gx_reset)
  bool cpxReady = false;
  bool cpxUsed = false;           // k_cpx_insert ran since the last gx_reset
  u32 cpxLastCapLog = 0;          // log2 of the capacity the last pass used (gx_complexity_last)
  // lengths and chromosome tallies of the kept samples' intervals (gx_interval_stats / gx_interval_stats_events, gx_ivstat.h);
  // nothing here exists before the first call
  struct IvsResult {
    int rep = 0;
    bool ctrl = false;
    u64 nInv = 0, wInv = 0;                 // the intervals that end before they start, their weight
    std::vector<uint64_t> len, n, w;        // sparse: n[i] intervals of length len[i] (ascending), their weight
    std::vector<uint64_t> cn, cw, cb;       // [nChrom] intervals, weight, sum of w L
  };
  DevBuf ivsOut, ivsBig;          // the control words + the counters; the list of long lengths
  std::vector<IvsResult> ivs;     // the last gx_interval_stats, per kept sample (until gx_reset)
  bool ivsReady = false;
  bool ivsUsed = false;           // k_ivstat ran since the last gx_reset
  size_t ivsLastCap = 0;          // the last pass: the list capacity it ended with, how often it ran again (gx_interval_stats_last)
  u32 ivsLastReruns = 0;
  // the strand cross-correlation of every closed sample's tags (gx_set_xcor / gx_push_tags, gx_xcor.h); nothing here exists
  // before gx_set_xcor turns it on; the results live on the host
  struct XcResult {
    int rep = 0;
    bool ctrl = false;
    u64 N = 0, nP = 0, nM = 0, rejected = 0;   // bases of the chromosomes that take part, set bits per strand, tags that were refused
    std::vector<uint64_t> n11;                 // [hi - lo + 1]
  };
  bool xcOn = false;
  int xcLo = 0, xcHi = -1;
  bool xcDirty = false;             // the table changed since the layout (gx_set_chroms / gx_set_owned)
  std::vector<XcChrom> xcChrom;     // the layout, and who takes part in the open sample
  u64 xcWords = 0;                  // words of one vector
  DevBuf xcPlus, xcMinus, xcTab, xcOut, xcTags;   // the two vectors, the table, the control words + n11, gx_push_tags' device buffer
  PinnedBuf xcStage[2];             // pinned staging of gx_push_tags (the caller's buffer is free on return)
  hipEvent_t xcStageFree[2] = {nullptr, nullptr};
  int xcStageNext = 0;
  std::vector<XcResult> xc;         // until gx_reset
  bool xcUsed = false;              // k_xc_set / k_xc_corr ran since the last gx_reset
  // the reference sequence as two bit vectors, GC bias per kept sample and GC content per interval (gx_set_genome /
  // gx_push_sequence / gx_gc_bias / gx_gc_content, gx_gcbias.h); nothing here exists before gx_set_genome turns it on
  struct GcResult {
    int rep = 0;
    bool ctrl = false;
    u32 W = 0;
    u64 fUn = 0, nUn = 0, wUn = 0;             // windows, intervals and weight that are not classed
    std::vector<uint64_t> F, Nn, Nw;           // [W + 1]
  };
  bool gcOn = false;
  bool gcDirty = false;             // the table changed since the layout (gx_set_chroms / gx_set_owned): laid out again, and empty
  bool gcDirDirty = false;          // bases were pushed since the directory was built
  std::vector<GcChrom> gcChrom;     // the layout
  std::vector<uint64_t> gcPushed;   // per chromosome: the end of the furthest push
  u64 gcWords = 0;                  // words of one vector
  DevBuf gcVec, gcAcgt, gcDir, gcTab, gcSeq, gcOut;   // the two vectors, the directory, the table, gx_push_sequence's device buffer, a pass's counters
  DevBuf gcAux;                     // a pass's small input: k_gc_expected's spans, k_gc_content's regions
  PinnedBuf gcStage[2];             // pinned staging of gx_push_sequence (the caller's buffer is free on return)
  hipEvent_t gcStageFree[2] = {nullptr, nullptr};
  int gcStageNext = 0;
  std::vector<GcResult> gcRes;      // the last gx_gc_bias, per kept sample (until gx_reset)
  bool gcReady = false;
  bool gcUsed = false;              // a kernel of gx_gcbias.h ran since the last gx_reset
  // the sequence itself and the motifs scanned in it (gx_set_genome_bases / gx_set_motifs / gx_motif_scan_*, gx_motifs.h);
  // nothing here exists before gx_set_genome_bases, gx_set_motifs and the first scan
  bool seqOn = false;               // the third vector exists: gx_push_sequence fills all three (k_seq_pack3)
  DevBuf gcAg;                      // ... laid out and cleared with the other two
  DevBuf seqOut;                    // gx_get_sequence's letters
  std::vector<MotMeta> motMeta;     // the motifs (gx_set_motifs) ...
  std::vector<int> motTabs;         // ... and their tables [motif][MOT_TAB_WORDS], both strands packed
  bool motDirty = false;            // ... are not on the device yet
  DevBuf motTabDev, motMetaDev, motReg, motOut, motList;   // tables, metas, a pass's regions, its control words and counts, its hit list
  PinnedBuf motHost;                // the count-only pass' words on their way back
  std::vector<gx_motif_hit> motHits;            // the last gx_motif_scan_peaks' hits, sorted (until gx_reset)
  std::vector<uint64_t> motCounts;              // ... and its counts [3][motif]
  bool motReady = false;
  bool motUsed = false;             // k_motif_scan ran since the last gx_reset
  u32 motLastReruns = 0, motLastBatches = 0;    // the last pass: how often it ran again, its LDS batches
  // every k-mer of the peaks and of the genome counted (gx_kmer_count_*, gx_kmers.h); nothing here exists before the first pass
  DevBuf kmTable, kmOut, kmReg;     // the 4^k counters in table-index order, the control words, a pass's regions
  PinnedBuf kmHost;                 // the table and the control words on their way back
  std::vector<uint64_t> kmCounts;   // the last gx_kmer_count_peaks' counts in the public order (until gx_reset) ...
  uint64_t kmWindows = 0, kmRegions = 0;   // ... its windows and the regions that hold at least k bases
  u32 kmK = 0;
  bool kmReady = false;
  bool kmUsed = false;              // k_kmer_count ran since the last gx_reset
  bool kmForceHbm = false;          // gx_kmer_force_hbm: every k takes the global-atomic path (for measurements)
  bool kmLdsSet = false;            // the LDS instance may take 64 KiB
  u32 kmLastPath = 0, kmLastFlushes = 0;   // the last pass: 0 LDS, 1 HBM; the flushes before a workgroup's end
  // the depth distribution of every closed sample's pileup (gx_set_depth_hist, gx_depth.h); the results live on the host
  struct DepthResult {
    int rep = 0;
    bool ctrl = false;
    u64 total = 0, excluded = 0, zero = 0;   // bases of the chromosomes that count, those inside -E regions, those at pileup 0
    u64 minV = 0, maxV = 0;                  // the smallest and the largest pileup above 0 (0: none)
    std::vector<uint64_t> bases, rsum, rsq;  // [DEPTH_BOUND] per whole depth
    std::vector<uint64_t> deepV, deepBases;  // the deep list: one entry per distinct v, ascending
  };
  bool depthOn = false;
  std::vector<DepthResult> depth;   // until gx_reset
  DevBuf depthOut, depthDeep;       // the control words + the three arrays; the deep list
  bool depthUsed = false;           // k_depth_hist ran since the last gx_reset
  size_t depthLastCap = 0;          // the last pass: the list capacity it ended with, how often it ran again (gx_depth_last)
  u32 depthLastReruns = 0;
  // each kept sample's depth inside the called peaks (gx_peak_signal / gx_peak_signal_events, gx_peaksig.h); nothing here exists
  // before the first call
  DevBuf psigSpace, psigRes;      // the peak space (one, cleared for sample after sample) and the records [sample][peak]
  PinnedBuf psigHost, psigEvHost; // the last gx_peak_signal's records (until gx_reset); the last gx_peak_signal_events'
  size_t psigPk = 0;              // peaks of the last gx_peak_signal
  bool psigReady = false;
  // the summits of the pooled treatment depth inside the called peaks (gx_peak_summits / gx_peak_summits_events, gx_summits.h):
  // the peak space is psigSpace (each pass drains the stream); nothing here exists before the first call
  DevBuf sumOut, sumFlag, sumList;            // the control words, the flagged peaks' run totals [peak], the summit list
  DevBuf sumBig, sumScrStart, sumScrVal, sumScrBlk;   // the second launch: the flagged peaks, the HBM scratch of their runs and blocks
  PinnedBuf sumMaxHost;                       // the samples' maxima, when the pooled events alone do not settle the domain
  std::vector<gx_summit> sumRes;              // the last gx_peak_summits' summits, by (peak, pos) (until gx_reset)
  bool sumReady = false;
  u32 sumLastReruns = 0, sumLastBig = 0;      // the last pass: how often it ran again, the peaks its second launch took
  // subsamples of the kept samples' events and the peak saturation curve (gx_subsample_*, gx_saturation, gx_subsample.h);
  // nothing here exists before the first call
  DevBuf subCnt, subOff;          // k_sub_count's counts per block, k_sub_scan's offsets
  DevBuf subOut;                  // gx_subsample_events' output
  std::vector<DevBuf> subBufs;    // kept sample k's subsample: the child reads it in place until its gx_sample_end
  bool subUsed = false;           // k_sub_write ran since the last gx_reset
  gx_ctx* satChild = nullptr;     // the context gx_saturation re-calls the peaks on (until gx_reset / gx_destroy)
  std::vector<gx_sat_point> satPts;             // the last gx_saturation, per point (until gx_reset)
  std::vector<std::vector<gx_peak>> satPeaks;   // ... and its peaks
  bool splitUsed = false;         // k_sub_split ran since the last gx_reset
  std::vector<gx_repro_call> reproCalls;        // the last gx_reproducibility, per call (until gx_reset)
  std::vector<std::vector<gx_peak>> reproPeaks; // ... and its peaks
  uint64_t reproSeed = 0;                       // ... and its seed
  // timing
  std::vector<Phase> phases;
  size_t nPhases = 0;
  std::vector<float> phaseMs;
  std::string phaseNames;
};

#define HIPCHECK(x)                                                                      \
  do {                                                                                   \
    hipError_t e__ = (x);                                                                \
    if (e__ != hipSuccess) {                                                             \
      ctx->err = std::string(#x) + ": " + hipGetErrorString(e__);                        \
      return GX_ERR_DEVICE;                                                              \
    }                                                                                    \
  } while (0)

namespace {

// buffer of at least `bytes`, recycled from the context's pool when possible
hipError_t pooled(gx_ctx* ctx, DevBuf& b, size_t bytes) {
  if (b.cap >= bytes) return hipSuccess;
  if (b.p) ctx->pool.push_back(std::move(b));
  int best = -1;
  for (int i = 0; i < (int)ctx->pool.size(); i++)
    if (ctx->pool[i].cap >= bytes && (best < 0 || ctx->pool[i].cap < ctx->pool[best].cap)) best = i;
  if (best >= 0) {
    b = std::move(ctx->pool[best]);
    ctx->pool.erase(ctx->pool.begin() + best);
    return hipSuccess;
  }
  return b.ensure(bytes);
}
void recycle(gx_ctx* ctx, DevBuf& b) {
  if (b.p) ctx->pool.push_back(std::move(b));
}

// pooled() failed: the runtime's sticky error is cleared, the context says "Cannot allocate memory"
int pool_failed(gx_ctx* ctx) {
  (void)hipGetLastError();
  ctx->err = "Cannot allocate memory";
  return GX_ERR_MEM;
}
// a call that is refused with its sentence
int refuse(gx_ctx* ctx, std::string why) {
  ctx->err = std::move(why);
  return GX_ERR_ORDER;
}
#define POOLED(ctx, buf, bytes)                                                          \
  do {                                                                                   \
    if (pooled(ctx, buf, bytes) != hipSuccess) return pool_failed(ctx);                  \
  } while (0)

// misc device words (u32 indices into ctx->misc)
enum { M_TICKET = 0, M_NIV = 1, M_BHCOUNT = 5, M_ALLONE = 6, M_BHOVF = 7, M_GENOME = 10 /* u64 */, M_NMERGED = 15, M_PSTAR = 14, M_VQ = 12 /* two words: k_bh_small */,
       // the sweep's counters are contiguous: one memset clears them
       M_TICKET2 = 16, M_SWCOUNT = 17, M_NPEAKS = 18, M_TICKET3 = 19, M_TICKET4 = 20, M_NHEADS = 21, M_PEAKBP = 22 /* u64 */,
       M_SWEEP_FIRST = 16, M_SWEEP_WORDS = 8, M_WORDS = 32 };
// the words of the nWide block (u32; in the zero arena: k_build_init clears them for every sample)
enum { NW_WIDE = 0,        // tiles on wideList (k_tile_meta)
       NW_HOT = 1,         // a base can reach the reference's int16 limits (level 1 of the sort, k_sbtile, k_hot_check)
       NW_HEAVY = 2,       // tiles on heavyList
       NW_CLOSE_TICKET = 8,   // k_scan_iv_close: its workgroups' counter
       NW_NEED_PAGES = 12, // the pages the longest level-1 list asked for (k_scan_bins: RETRY_PT sizes the table by it)
       NW_NBIG = 13,       // bins k_sbtile's first launch left to its second
       NW_SBT_TICKET = 14 };  // k_sbtile's first launch: the bin counter of its persistent workgroups
u32* nw_word(const gx_ctx* ctx, int w) { return ctx->nWide.as<u32>() + w; }

// GX_DEBUG=1: synchronise after every launch and say which kernel it was (hang / fault triage)
// the grid of a kernel whose wavefronts stride over the tiles, four to a workgroup: at most perCU workgroups per CU
dim3 tile_grid(const gx_ctx* ctx, int perCU) { return dim3(std::max(1u, std::min((ctx->nTiles + 3) / 4, (u32)(perCU * ctx->numCU)))); }

// -q on the loose slots may be taken at all (one replicate without a control is gx_find_peaks' to see: plan_call): asked by
// plan_build (the late bits are only wanted for it), gx_pvalues and plan_call.  k_bh_small inserts up to PV_WHOLE keys with an
// unbounded probe: the table must have room for all of them (GX_BH_CAPLOG may start it smaller; the tight path grows it)
bool q_loose_may(const gx_ctx* ctx) {
  return ctx->par.qval_opt && !ctx->knob.noQLoose && !ctx->qLooseBad && !ctx->sawFrac && !ctx->knob.noPackHist &&
         (1u << ctx->bhCapLog) >= 2u * PV_WHOLE;
}

int dbg_sync(gx_ctx* ctx, const char* what) {
  if (!ctx->knob.debug) return GX_OK;
  fprintf(stderr, "[gx] %s ...", what);
  fflush(stderr);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  fprintf(stderr, " %s\n", e == hipSuccess ? "ok" : hipGetErrorString(e));
  fflush(stderr);
  if (e != hipSuccess) {
    ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return GX_ERR_DEVICE;
  }
  return GX_OK;
}

// phase timers: the event pairs are created once and reused run after run
// (an event record costs a ~5 us bubble on the stream: gx_set_phase_timing chooses none / the tile stage / all)
static bool phase_wanted(const gx_ctx* ctx, const char* name) {
  if (ctx->phaseLevel >= 2) return true;
  if (ctx->phaseLevel != 1) return false;
  const char* base = name[0] && name[1] == '.' ? name + 2 : name;  // "t.tile" / "c.tile" -> "tile"
  return ctx->phaseFilter == base;
}
// roctx ranges ("roctx ranges per phase"): host-side markers of the profiler, opened at run time like RCCL --
// librocprofiler-sdk-roctx is what rocprofv3 --marker-trace listens to, libroctx64 its predecessor.  Absent: no ranges.
struct RoctxApi {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
};
static const RoctxApi* roctx_api() {
  static RoctxApi api;
  static std::once_flag once;
  std::call_once(once, [&]() {
    for (const char* n : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
      void* h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
      if (!h) continue;
      api.push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
      api.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
      if (api.push && api.pop) break;
      api.push = nullptr;
      api.pop = nullptr;
    }
  });
  return api.push ? &api : nullptr;
}
void phase_begin(gx_ctx* ctx, const char* name) {
  if (ctx->knob.roctx)
    if (const RoctxApi* r = roctx_api()) {
      char buf[48];
      snprintf(buf, sizeof buf, "gx:%s", name);
      (void)r->push(buf);
      ctx->roctxOpen = true;
    }
  ctx->phaseOpen = phase_wanted(ctx, name);
  if (!ctx->phaseOpen) return;
  if (ctx->nPhases == ctx->phases.size()) {
    Phase ph;
    (void)hipEventCreate(&ph.a);
    (void)hipEventCreate(&ph.b);
    ctx->phases.push_back(ph);
  }
  Phase& ph = ctx->phases[ctx->nPhases++];
  ph.name = name;
  (void)hipEventRecord(ph.a, ctx->stream);
}
void phase_end(gx_ctx* ctx) {
  if (ctx->phaseOpen) (void)hipEventRecord(ctx->phases[ctx->nPhases - 1].b, ctx->stream);
  ctx->phaseOpen = false;
  if (ctx->roctxOpen) {
    (void)roctx_api()->pop();
    ctx->roctxOpen = false;
  }
}

int status_to_rc(gx_ctx* ctx, u32 st) {
  ctx->statusSeen |= st;  // (gx_reset clears the device word only when something was ever raised)
  if (!st) return GX_OK;
  struct { u32 bit; int rc; const char* msg; } tab[] = {
      {ST_LOOKBACK, GX_ERR_DEVICE, "look-back / page-table spin limit reached"},
      {ST_BAD_CHROM, GX_ERR_ORDER, "event on an unknown chromosome"},
      {ST_BAD_POS, GX_ERR_POS, ": read aligned beyond reference end"},
      {ST_BAD_COUNT, GX_ERR_ALNS, "Disallowed number of alignments"},
      {ST_NEG_PILE, GX_ERR_PILE, "Invalid pileup value (< 0)"},
      {ST_NO_FRAGS, GX_ERR_EXPT, "Experimental sample has no analyzable fragments"},
      {ST_HASH_FULL, GX_ERR_DEVICE, "p-value table full"},
      {ST_BAD_DF, GX_ERR_DF, "Invalid df in pchisq()"},
      {ST_PT_FULL, GX_ERR_MEM, "level-1 page table full"},
      {ST_END_PILE, GX_ERR_ARR, "pileup of a chromosome does not return to 0 behind its last base"},
      {ST_BH_LEN, GX_ERR_PVAL, "Genome length does not match p-value length"},
  };
  for (auto& t : tab)
    if (st & t.bit) {
      ctx->err = t.msg;
      return t.rc;
    }
  ctx->err = "unknown device status";
  return GX_ERR_DEVICE;
}

int read_status(gx_ctx* ctx) {
  HIPCHECK(hipMemcpyAsync(&ctx->mail->status, ctx->dStatus.p, sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  return status_to_rc(ctx, ctx->mail->status);
}

// ---- risky p-values (gx_math.h round_checked; gx_kernels.h RiskBuf) --------------------------------
// mail_sync: at a synchronisation the host needs anyway, the list's count and first records come along.
// risk_apply: after it, evaluate the listed values with the host's libm and send them back (k_risk_apply).
// One small kernel writes everything the host wants to know into pinned memory (scalars, status, flags, the
// risky list's count and first records), then the stream is synchronised.  Null pointers: not wanted.
// The host does not wait in hipStreamSynchronize (an interrupt and a wake-up: 20-30 us after the kernel): k_mail
// writes a sequence number behind everything else and the host polls that word in pinned memory (a few us).  After
// 20 ms of polling -- or with GX_NO_SPIN -- it blocks in the runtime after all, which also reports a device fault.
MailOut mail_out(gx_ctx* ctx) {
  HostMail* dm = static_cast<HostMail*>(ctx->mailBuf.dp);
  return MailOut{&dm->scal, &dm->status, &dm->hot, &dm->nIv, &dm->coll[2], &dm->nMerged, reinterpret_cast<u64*>(&dm->peakBP),
                 static_cast<RiskBuf*>(ctx->riskHost.dp), &dm->seq};
}

int mail_wait(gx_ctx* ctx, u32 seq);

int mail_sync(gx_ctx* ctx, const Scalars* ds, const u32* hot, const u32* nIv, const long long* coll, const u32* extra,
              const u64* extra64 = nullptr) {
  const u32 seq = ++ctx->mailSeq;
  hipLaunchKernelGGL(k_mail, dim3(1), dim3(64), 0, ctx->stream, ds, ctx->dStatus.as<u32>(), hot, nIv, coll, extra,
                     ctx->dRisk.as<RiskBuf>(), mail_out(ctx), seq, extra64);
  HIPCHECK(hipGetLastError());  // (a launch that failed is reported now, not after the polling gives up)
  return mail_wait(ctx, seq);
}

// (the mail kernel -- k_mail, or k_scan_iv_close -- has been launched with this sequence number)
int mail_wait(gx_ctx* ctx, u32 seq) {
  const bool spin = !ctx->knob.noSpin;
  volatile u32* word = &ctx->mail->seq;
  if (spin) {
    const auto t0 = std::chrono::steady_clock::now();
    for (u32 it = 0; *word != seq; it++) {
      __builtin_ia32_pause();
      if ((it & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
  }
  if (*word != seq) HIPCHECK(hipStreamSynchronize(ctx->stream));
  std::atomic_thread_fence(std::memory_order_acquire);
  return GX_OK;
}

struct RiskHostIn { const float* a; const float* b; };  // RK_SELF: the caller's inputs

float risk_host_value(const gx_ctx* ctx, const RiskRec& r, const RiskHostIn& in) {
  const float lambda = ctx->hScal.lambda, factor = ctx->hScal.factor;
  bool ng = false, rk = false;
  switch (r.kind) {
    case RK_LUT:
    case RK_DEEP: return calc_pval(getval((int)r.a, &ng), lambda, &rk);  // no control: the control value is lambda
    case RK_TAB2D:
      return calc_pval((float)(r.a / PT_N), ctrl_net((int)((r.a % PT_N) * GX_UNIT), factor, lambda, &ng), &rk);
    case RK_PAIR: return calc_pval(expt_val((int)r.b, &ng), ctrl_net((int)r.c, factor, lambda, &ng), &rk);
    case RK_FISHER: return fisher_combine(r.x, (int)r.c, &rk);
    case RK_SELF:
      if (r.b == 1) return calc_pval(in.a[r.a], in.b[r.a], &rk);
      if (r.b == 3 || r.b == 4) return fisher_combine((double)in.a[r.a], (int)in.b[r.a], &rk);
      return 0.0f;
    default: return 0.0f;
  }
}

int risk_apply(gx_ctx* ctx, RiskTargets T, RiskHostIn in = RiskHostIn{nullptr, nullptr}) {
  RiskBuf* hb = static_cast<RiskBuf*>(ctx->riskHost.p);
  const u32 n = hb->count;
  if (!n) return GX_OK;
  hipStream_t s = ctx->stream;
  if (n > RISK_CAP) {
    HIPCHECK(hipMemsetAsync(ctx->dRisk.p, 0, 4, s));
    ctx->err = "more p-values next to a float rounding boundary than the list holds";
    return GX_ERR_DEVICE;
  }
  if (n > RISK_PREFIX) {  // (rare: the count and the first records came with the synchronisation already paid for)
    HIPCHECK(hipMemcpyAsync(hb->rec + RISK_PREFIX, ctx->dRisk.as<RiskBuf>()->rec + RISK_PREFIX,
                            (size_t)(n - RISK_PREFIX) * sizeof(RiskRec), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
  for (u32 i = 0; i < n; i++) {
    const float pn = risk_host_value(ctx, hb->rec[i], in);
    hb->rec[i].pnew = pn;
    // (the tile stage compared the device's table entry, one float away at most, with the threshold: LooseCtl)
    const float thr = ctx->par.thr;
    if (hb->rec[i].kind == RK_LUT && ((pn > thr) != (nextafterf(pn, -INFINITY) > thr) || (pn > thr) != (nextafterf(pn, INFINITY) > thr)))
      ctx->riskNearThr = true;
  }
  // (the pinned records stay untouched until the next mail_sync)
  // A short list is read by the kernel where it lies (mapped pinned memory): no copy launch.
  const RiskRec* src = static_cast<const RiskBuf*>(ctx->riskHost.dp)->rec;
  if (n > RISK_PREFIX) {
    HIPCHECK(hipMemcpyAsync(ctx->dRisk.as<RiskBuf>()->rec, hb->rec, (size_t)n * sizeof(RiskRec), hipMemcpyHostToDevice, s));
    src = ctx->dRisk.as<RiskBuf>()->rec;
  }
  T.lutP = ctx->pvLut.as<float>();
  T.p2d = ctx->pairP2d.as<float>();
  T.deep = ctx->dDeep.as<DeepTab>();
  hipLaunchKernelGGL(k_risk_apply, dim3(1), dim3(256), 0, s, ctx->dRisk.as<RiskBuf>(), src, n, T);
  hb->count = 0;
  return dbg_sync(ctx, "k_risk_apply");
}

}  // namespace
