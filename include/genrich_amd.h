/*
 * genrich_amd.h -- C ABI of the MI355X-native Genrich hot path.
 *
 * The reference (jsh58/Genrich v0.6.2) is a monolith with no plugin/FFI
 * interface; this header is the drop-in boundary cut where its data narrows
 * (SURVEY.md section 8b).  Every entry point names the reference code it
 * replaces (file:line into Genrich.c / Genrich.h).  Plain C types only: no
 * torch, no HIP types.  Handle based, not thread-safe (the reference is
 * single-threaded, README.md:535).
 *
 * Call order for one run (mirrors runProgram, Genrich.c:5386-5607):
 *
 *   gx_create -> gx_set_chroms
 *   for each replicate:
 *     gx_sample_begin(ctx, 0, save) ; gx_push_events* ; gx_sample_end   (treatment)
 *     either  gx_sample_begin(ctx, 1, NULL) ; gx_push_events* ; gx_sample_end   (control)
 *     or      gx_sample_no_control
 *     gx_pvalues
 *   gx_find_peaks -> gx_get_peaks / gx_get_intervals
 *   (counting on: gx_count_in_peaks -> gx_get_peak_counts / gx_write_counts)
 *   (coverage on, any time after a gx_sample_end: gx_get_coverage / gx_write_coverage)
 *   (profile on, any time after a gx_sample_end: gx_get_profile / gx_write_profile_group)
 *   (depth on, any time after a gx_sample_end: gx_get_depth / gx_write_depth_group)
 *   (coverage on, between samples or after them: gx_coverage_gram / gx_write_correlation_group)
 *   (coverage on, between samples or after them: gx_coverage_fingerprint / gx_write_fingerprint_group)
 *   gx_destroy
 */
#ifndef GENRICH_AMD_H
#define GENRICH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GX_SKIP (-1.0f) /* Genrich.h:27  SKIP: statistic of an excluded (-E) region */

/* Status codes.  0 = success; negative values map 1:1 onto the reference's
 * errCode enum (Genrich.h:97-106) so a host can print the identical
 * "Error! <msg>" text (Genrich.c:78-81) and exit(1). */
enum gx_status {
  GX_OK = 0,
  GX_ERR_MEM = -1,      /* ERRMEM    "Cannot allocate memory" */
  GX_ERR_GEN = -2,      /* ERRGEN    "No analyzable genome (length=0)"           Genrich.c:1828 */
  GX_ERR_EXPT = -3,     /* ERREXPT   "Experimental sample has no analyzable fragments" :2292 */
  GX_ERR_PILE = -4,     /* ERRPILE   "Invalid pileup value (< 0)"                :1921,1969 */
  GX_ERR_POS = -5,      /* ERRPOS    ": read aligned beyond reference end"       :2531 */
  GX_ERR_ALNS = -6,     /* ERRALNS   "Disallowed number of alignments"           :2402,2485 */
  GX_ERR_ARR = -7,      /* ERRARR / ERRARRC / "finishes at %f (not 0.0)"         :2144,2276,2153,2284 */
  GX_ERR_PVAL = -8,     /* ERRPVAL / genome-length mismatch                      :344,377 */
  GX_ERR_DF = -9,       /* ERRDF     "Invalid df in pchisq()"                    :556 */
  GX_ERR_ORDER = -10,   /* API called out of order / bad argument */
  GX_ERR_DEVICE = -11   /* HIP runtime failure (message via gx_last_error) */
  /* (-12 was GX_ERR_OVERFLOW until round 5; the reference's int16 saturation skips, Genrich.c:2558-2573, are
   * reproduced -- gx_filter_saturation -- so nothing reports it: retired, the number is not reused) */
};

/* One alignment-derived interval AFTER saveInterval's clamping
 * (Genrich.c:2522-2544): 0 <= start < len(chrom), start <= end <= len.
 * weight = 1/count, count in {1,2,3,4,5,6,8,10} (Genrich.c:2576-2583,
 * addFrac 2311, subFrac 2412). */
typedef struct gx_event {
  uint32_t chrom; /* index into the table given to gx_set_chroms */
  uint32_t start;
  uint32_t end;
  uint32_t count;
} gx_event;

/* Peak-calling parameters: the tail of runProgram's argument list
 * (Genrich.c:5390-5395) after getArgs' conversions (5796-5817). */
typedef struct gx_params {
  float thr;           /* minPQval = -log10f(-p or -q value)           Genrich.c:5817 */
  int32_t qval_opt;    /* 1: significance on q-values (-q)             :5790 */
  float min_auc;       /* -a, DEFAUC 200.0f                            Genrich.h:31 */
  int32_t min_len;     /* -l, DEFMINLEN 0 */
  int32_t max_gap;     /* -g, DEFMAXGAP 100 */
  int32_t device;      /* HIP device ordinal (ignored by the CPU oracle) */
  uint64_t genome_len; /* -L, 0 = compute from the chromosome table    :1819,1091 */
} gx_params;

/* One called peak = the arguments of printPeak (Genrich.c:885-887). */
typedef struct gx_peak {
  uint32_t chrom;
  uint32_t start;
  uint32_t end;
  uint32_t summit; /* offset of the summit from start (narrowPeak column 10) */
  float auc;       /* signal (column 7) */
  float p;         /* summit -log10 p (column 8) */
  float q;         /* summit -log10 q (column 9) or GX_SKIP without -q */
} gx_peak;

typedef struct gx_ctx gx_ctx;

/* ---- life cycle ------------------------------------------------------- */

int gx_create(gx_ctx** ctx, const gx_params* params);
void gx_destroy(gx_ctx* ctx);
/* Forget all replicates and results but keep the chromosome table and device buffers
 * (a fresh run without re-allocating; what the reference does by exiting the process). */
int gx_reset(gx_ctx* ctx);
const char* gx_last_error(const gx_ctx* ctx);
const char* gx_strerror(int status); /* the reference's errMsg text, Genrich.h:107-154 */

/* Chromosome table in header order = output order (saveChrom, Genrich.c:4220-4270).
 * skip[i]   : chromosome listed in -e (Chrom.skip, :4243).
 * bed[i]    : merged, sorted -E coordinates as start/end pairs (Chrom.bed, saveXBed :1144);
 *             bed_len[i] = number of coordinates (even). bed/bed_len may be NULL. */
int gx_set_chroms(gx_ctx* ctx, int n, const uint32_t* len, const uint8_t* skip,
                  const uint32_t* const* bed, const int32_t* bed_len);

/* ---- per-sample event stream (replaces saveInterval's accumulate step,
 *      Genrich.c:2546-2583, and the re-zeroing of diff arrays, :5503-5510) ---- */

/* is_ctrl = 0: start the treatment file of the next replicate; save[i] = chromosome
 * appears in this treatment file's header (Chrom.save, :4230-4244, reset :5463).
 * is_ctrl = 1: start the matching control file (save must be NULL). */
int gx_sample_begin(gx_ctx* ctx, int is_ctrl, const uint8_t* save);

/* Host-resident events; consumed before return (the caller may reuse its buffer at once).  They go through
 * two pinned staging buffers and asynchronous copies on a side stream: the call does not wait for the
 * upload, so the host parses the next batch while this one travels, and gx_sample_end starts its first
 * kernel on the pieces that have arrived while the rest is still on its way. */
int gx_push_events(gx_ctx* ctx, const gx_event* events, size_t n);

/* The same for a caller whose buffer is page-locked (hipHostMalloc / hipHostRegister) and stays untouched
 * until gx_sample_end: the upload reads it in place, no staging copy. */
int gx_push_events_pinned(gx_ctx* ctx, const gx_event* events, size_t n);

/* Events already resident in device memory (HIP path only; the pointer must stay
 * valid until gx_sample_end -- with gx_set_count_in_peaks on, until the run's last gx_count_in_peaks). */
int gx_push_events_device(gx_ctx* ctx, const gx_event* d_events, size_t n);

/* The same event in 8 bytes (round 6): what saveInterval receives (Genrich.c:2516-2519) is a start, a length that a read pair
 * bounds, one of eight weights and a chromosome -- 16 bytes of gx_event are the step's largest stream (0.8 GB for 50 M
 * fragments) and twice what PCIe has to carry.
 *   start : as gx_event's
 *   lcc   : [15:0] end - start (< 65535);  [18:16] count class 0..7 = count 1, 2, 3, 4, 5, 6, 8, 10;  [31:19] chromosome (< 8192)
 * An event that does not fit (65,535 bases or more, an end before its start, a chromosome index of 8192 or more) travels as a
 * gx_event through gx_push_events; the two calls may be mixed within a sample in any order (the pileup is a sum; only the
 * replay of the reference's int16 decisions, gx_filter_saturation, looks at the order, and takes the pushes as they came).
 * gx_event8_pack: 1 and *out when `in` fits, 0 otherwise (host helper, no context).
 * where: GX_EVENTS_HOST (pageable memory, consumed before return), GX_EVENTS_PINNED (page-locked, untouched until
 * gx_sample_end), GX_EVENTS_DEVICE (device memory, valid until gx_sample_end; a 16-byte aligned buffer is read in place). */
typedef struct gx_event8 {
  uint32_t start;
  uint32_t lcc;
} gx_event8;
#define GX_EVENTS_HOST 0
#define GX_EVENTS_PINNED 1
#define GX_EVENTS_DEVICE 2
int gx_event8_pack(const gx_event* in, gx_event8* out);
int gx_push_events_packed(gx_ctx* ctx, const gx_event8* events, size_t n, int where);

/* The reference's int16 saturation rule (Genrich.c:2558-2573): saveInterval drops an alignment
 * when the int16 part of diff[start] already holds INT16_MAX or that of diff[end] INT16_MIN, which
 * depends on the order of the alignments.  keep[i] = 0 for the events (in input order, as for
 * gx_push_events; lengths as for gx_set_chroms) that it would drop, 1 otherwise.  Host-only: no
 * context, no device.  gx_sample_end applies the same rule itself when the device finds a base
 * that can saturate at all.  Returns the number of events dropped, or a negative gx_status. */
long long gx_filter_saturation(const gx_event* events, size_t n, int n_chrom, const uint32_t* len, uint8_t* keep);

/* The OPEN sample's difference array on [pos0, pos0 + n) of one chromosome, from the events pushed so far (between
 * gx_sample_begin and gx_sample_end): net[i] = weight, in 1/120 units, of the events that start at pos0 + i minus the
 * weight of those that end there -- the exact value of saveInterval's diff[pos0 + i] (Genrich.c:2576-2583; an end beyond
 * the chromosome counts at its length, 2536-2544, so pos0 + i may be the length itself; events that gx_sample_end would
 * reject are left out).  For a caller that needs saveInterval's int16 decisions READ BY READ -- the -v warnings
 * "skipped due to overflow / underflow", the missing -b line, the length 0 towards the -x average (2558-2573) --
 * and not only their effect on the pileup (which gx_sample_end reproduces by itself): it counts starts and ends per
 * window as it pushes, asks for a window's exact state when one comes near 32,767, and keeps that window itself from
 * then on (genrich_amd/host/host_state.h: HotWindows).  One pass over the pushed events; waits for their uploads.
 * n <= 65536. */
int gx_window_net(gx_ctx* ctx, uint32_t chrom, uint32_t pos0, uint32_t n, long long* net);

/* PCR duplicates (-r): the membership half of findDupsPr / findDupsDc / findDupsSn (Genrich.c:3616-3690, 3761-3880, 3886-3944;
 * a discordant combination is looked up in both orders of its ends and stored in one -- the table is keyed on the unordered
 * pair, so the host hands the two ends over in a canonical order; the tables'
 * keys are the fields jenkins_hash_aln hashes, 3408-3450, packed by the host into four words -- an alignment-type tag
 * with the chromosome(s), the 5' end(s), the strand(s)).  keys[0..n) are the alignments of a file's sets in the order
 * in which findDups visits them (highest quality sum first; anything added to a table unconditionally -- the ends of
 * kept pairs in the singleton table, checkAndAdd 3514 -- comes as a record like any other); multi[i] != 0 when record
 * i belongs to a set with several alignments.  owner[i] = index of the FIRST record with record i's key (i itself: the
 * key was free), with bit 31 set when some record with that key belongs to a multi-alignment set: a set of one
 * alignment whose owner word has no bit 31 is a duplicate exactly when owner[i] != i, and of the set owner[i] belongs
 * to; everything that carries bit 31 is left to the caller, who walks those few sets in order as the reference does.
 * n <= 2^30 (the table has 2^k >= 2 n slots addressed by 32-bit indices); a larger n, or a NULL array with n > 0, is
 * GX_ERR_ORDER before anything is allocated; n = 0 is GX_OK and leaves owner alone.  Uses the context's device and stream;
 * independent of the sample state.
 * gx_dups_geometry: what the table's edge cases depend on, host-only (no context, no device): *capacity = the slots
 * gx_dups_first uses for n records -- the least power of two that is >= 2 n and >= 1024 -- and home[i] = the slot at which the
 * probe of keys[i] starts in a table of that capacity (the kernels' own hash & (capacity - 1); a probe walks upwards from
 * there and wraps at the end).  capacity or home may be NULL; n > 2^30: GX_ERR_ORDER. */
typedef struct { uint32_t w[4]; } gx_dup_key;
int gx_dups_first(gx_ctx* ctx, const gx_dup_key* keys, const uint8_t* multi, size_t n, uint32_t* owner);
int gx_dups_geometry(const gx_dup_key* keys, size_t n, uint32_t* capacity, uint32_t* home);

/* Treatment: == savePileupExpt (Genrich.c:2168-2295), returns fragLen.
 * Control : == savePileupCtrl (:2052-2161), returns lambda and factor.
 * Any out pointer may be NULL. */
int gx_sample_end(gx_ctx* ctx, double* frag_len, float* lambda, float* factor);

/* How many alignments of the sample just closed (gx_sample_end) the reference's int16 saturation rule dropped
 * (Genrich.c:2558-2573; normally 0).  The library has dropped them as the reference does; a host program that
 * printed their -b lines or counted their lengths beforehand can at least say so. */
int gx_saturation_dropped(gx_ctx* ctx, long long* n);

/* == savePileupNoCtrl (Genrich.c:1883-1896): missing or "null" control. */
int gx_sample_no_control(gx_ctx* ctx, float* lambda);

/* == savePval (Genrich.c:1720-1794) for the current replicate; closes the replicate. */
int gx_pvalues(gx_ctx* ctx);

/* ---- genome-wide statistics and peaks (replaces findPeaks, Genrich.c:1076-1137:
 *      combinePval 612, computeQval 352, callPeaks 977) ---- */

int gx_find_peaks(gx_ctx* ctx, size_t* n_peaks, uint64_t* genome_len, uint64_t* peak_bp);

/* Copies min(cap, n_peaks) peaks, chromosome-table order then position. */
int gx_peak_count(gx_ctx* ctx, size_t* n_peaks);
int gx_get_peaks(gx_ctx* ctx, gx_peak* out, size_t cap);

/* Interval arrays for host-side -f / -k formatting (printLog 808, printPile 1697).
 * which: replicate index r (0..n-1) = that replicate's p-value intervals,
 *        GX_IV_FINAL = the intervals peaks were called on (combined when n > 1).
 * Arrays (any may be NULL) receive n_iv entries: end[], expt[] and ctrl[] pileups
 * (only meaningful for a single replicate, as in the reference), p[], q[].
 * q (with -q, GX_IV_FINAL only; saveQval 212-250): gx_find_peaks looks q up where updatePeak reads it -- inside the candidate
 * peaks -- and the whole array is made when it is first asked for here, from the run's {p -> q} table, which stays on the device
 * until the next gx_find_peaks of the context takes it (then: GX_ERR_ORDER for an array that was never asked for). */
#define GX_IV_FINAL (-1)
int gx_interval_count(gx_ctx* ctx, int which, int chrom, size_t* n_iv);
int gx_total_intervals(gx_ctx* ctx, int which, size_t* n_iv); /* over all chromosomes */
int gx_get_intervals(gx_ctx* ctx, int which, int chrom, size_t cap, uint32_t* end,
                     float* expt, float* ctrl, float* p, float* q);

/* ---- each sample's intervals counted in the called peaks (FRiP, a per-peak count matrix).  Genrich has NO counterpart:
 *      it prints the intervals (-b: saveInterval / printBED, Genrich.c:2516-2590) and forgets them.  ----
 * A sample = every gx_sample_end of the run, in call order: for replicate r its treatment, then its control when one was
 * read (even one without a usable record); gx_sample_no_control is none.  Its intervals are exactly those that entered its
 * pileup -- the lines -b prints for it: end clamped to the chromosome's length (2536-2544), after the int16 rule's drops
 * (2558-2573, gx_filter_saturation), none on -e chromosomes (2995) nor on chromosomes this context does not own, empty ones
 * included -- each with the weight 120 / count (1/120 units, gx_math.h).  Interval [s, e) overlaps peak [ps, pe) (narrowPeak
 * coordinates) iff s < pe && ps < e, and counts in every peak it overlaps.  Per sample, exact int64 sums in 1/120 units:
 * count[k] = weight of its intervals that overlap peak k (gx_get_peaks order), total = weight of all of them, in_peaks =
 * weight of those that overlap at least one peak; FRiP = in_peaks / total.
 *
 * gx_set_count_in_peaks: only while idle (after gx_create / gx_reset, before the first gx_sample_begin; else GX_ERR_ORDER);
 *   off by default.  It is the switch that keeps the events, for gx_count_in_peaks and gx_count_in_regions alike.  On, each
 *   closed sample keeps its events in device memory until gx_reset (which keeps the switch):
 *   the library's own copies (host pushes, 16-byte forms of packed pieces, the survivors of the int16 rule) are not reused
 *   for the next sample, and a caller's DEVICE buffer (gx_push_events_device, gx_push_events_packed(.., GX_EVENTS_DEVICE))
 *   is read in place, so it must stay valid and unchanged until the run's last gx_count_in_peaks (or gx_reset / gx_destroy)
 *   instead of until gx_sample_end.  Off, nothing is kept and nothing of a run changes.
 * gx_count_in_peaks: after gx_find_peaks (else GX_ERR_ORDER); counts every kept sample (*n_samples of them) in one device
 *   pass and one read-back; may be called again, with the same result.  Under gx_set_owned a context counts the chromosomes
 *   it owns (an interval and every peak it can touch lie on one chromosome): a host adds the contexts' totals.
 * gx_get_peak_counts: the last count of one sample (0 .. n_samples-1): its replicate, whether it is a control, min(cap,
 *   n_peaks) counts (count120 may be NULL when cap is 0) and the two totals (any pointer may be NULL). */
int gx_set_count_in_peaks(gx_ctx* ctx, int on);
int gx_count_in_peaks(gx_ctx* ctx, int* n_samples);
int gx_get_peak_counts(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, int64_t* count120, size_t cap, int64_t* total120,
                       int64_t* in_peaks120);

/* ---- counting in a given region set (no Genrich counterpart) ----
 * The same samples and the same intervals, with the same weights, as gx_count_in_peaks above, counted in regions the caller
 * names -- a common set for several runs -- instead of the peaks this run called.  Region k is (chrom, start, end), start <
 * end, in the caller's order; the set may overlap, nest, repeat and be unsorted.  Interval [s, e) on the same chromosome
 * overlaps it iff s < end && start < e (the predicate of the peaks) and counts in EVERY region it overlaps.  end may lie beyond
 * the chromosome's length; chrom >= n_chrom (a chromosome the run does not know), a skipped (-e) or un-owned chromosome and
 * start >= the chromosome's length are legal and count 0.  An interval that ends before it starts (convert_event lets them into
 * the pileup and the peak counts) is counted by the same predicate.  Per sample, exact int64 sums in 1/120 units: count[k],
 * total = the value gx_count_in_peaks reports, in_regions = weight of the intervals that overlap at least one region (the
 * union: an interval in three regions counts once).
 *
 * gx_count_in_regions: needs gx_set_count_in_peaks on and no sample open (else GX_ERR_ORDER); it needs no gx_pvalues,
 *   gx_find_peaks or peak.  Counts every sample closed so far (*n_samples of them, in gx_sample_end order) in one device pass
 *   and one read-back; may be called again, with other regions; n == 0 is legal.  A region with start >= end: GX_ERR_ORDER,
 *   and nothing is counted.  The last gx_count_in_peaks result stays readable and vice versa; gx_reset drops both.  Under
 *   gx_set_owned a context counts the chromosomes it owns: a host adds the contexts' rows and totals.
 * gx_get_region_counts: the last count of one sample: min(cap, n) counts in the regions' order and the two totals, as
 *   gx_get_peak_counts. */
typedef struct { uint32_t chrom, start, end; } gx_region;
int gx_count_in_regions(gx_ctx* ctx, const gx_region* regions, size_t n, int* n_samples);
int gx_get_region_counts(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, int64_t* count120, size_t cap, int64_t* total120,
                         int64_t* in_regions120);

/* ---- each sample's own signal inside the called peaks: height, summit, area (no Genrich counterpart: the replicates'
 *      p-values end in Fisher's sum, multPval Genrich.c:528-583, and the narrowPeak line does not say which replicate carries
 *      a peak; the usual route is bedtools map / multiBigwigSummary over per-sample tracks made in another pass) ----
 * The samples, their order, their intervals and their weights are exactly those of gx_count_in_peaks: every gx_sample_end of
 * the run in call order; the sample's -b lines, the end clamped to the chromosome's length, after -r and the int16 rule's
 * drops; weight 120 / count; nothing on -e, unsaved or un-owned chromosomes.  A sample's depth is the prefix sum of its
 * difference array, as the pileup is: +w at s, -w at the clamped e.  An interval with e == s adds nothing; one with e < s
 * (convert_event lets them in) adds -w over [e, s), as it does in the pileup.  -E regions are NOT masked: this is the depth of
 * the sample's intervals, the one place where it differs from the `experimental` column of -k, which is 0 inside them.
 * For sample i and peak k = [ps, pe) (gx_get_peaks order, narrowPeak coordinates), all exact signed int64 in 1/120 units
 * (summit and covered: bases):
 *     area120[k]      = the sum of depth(x) over x in [ps, pe)
 *     max120[k]       = the largest depth(x) there             summit[k] = the smallest x - ps at which it is reached
 *     covered[k]      = the bases of [ps, pe) with depth > 0
 *     at_summit120[k] = depth(ps + gx_peak.summit), the run's own summit base
 * No figure depends on the launch geometry, the order of the adds, the push mode (host, pinned, device, packed) or the number
 * of contexts: integer adds only.  Domain: the pileup's own, a depth below 2^31 (1/120 units) at every base.
 *
 * gx_peak_signal: after gx_find_peaks, with gx_set_count_in_peaks on (else GX_ERR_ORDER); every kept sample (*n_samples of
 *   them) through k_psig_scatter / k_psig_reduce (gx_peaksig.h) over ONE buffer of an int32 per peak base, cleared for every
 *   sample, and one read-back; may be called again, with the same result; no peak or no sample is legal.  Under gx_set_owned a
 *   context handles the peaks of the chromosomes it owns, as the count does.  The results of gx_count_in_peaks /
 *   gx_count_in_regions stay readable; gx_reset drops this one.  A failed allocation: GX_ERR_MEM.  Its phase is "peaksig"
 *   (gx_phase_times).  Nothing of it is allocated or launched before the first call.
 * gx_get_peak_signal: the last pass's figures of one sample (0 .. n_samples-1): its replicate, whether it is a control and
 *   min(cap, n_peaks) entries of each array.  Any pointer may be NULL.
 * gx_peak_signal_events: the same two kernels over n events in host memory (copied to the device by the call), all ONE sample
 *   whose save mask lists every chromosome of the context's table (after gx_set_chroms; -e and gx_set_owned hold as for a
 *   sample), in n_peaks peaks the caller gives: sorted by (chrom, start), disjoint (end <= the next start), not empty, inside
 *   their chromosomes, on chromosomes this context works on; summit_off[k] < end - start is the base at_summit120 reads (NULL:
 *   base 0).  Anything else, n >= 2^31 / 120 (as many unit intervals on one base leave the domain) or grid > 65535:
 *   GX_ERR_ORDER with a text before anything is allocated or launched.  grid = 0: the library's geometry, else that many
 *   workgroups for either kernel.  Each output holds n_peaks entries (any may be NULL).  No sample open.  For tests and
 *   measurements: constructed peaks that no small run calls; it leaves gx_get_peak_signal's result alone.
 * gx_peak_signal_geometry: what the edge cases depend on, without a device: the lanes of a workgroup of k_psig_reduce (a
 *   wavefront of 64 per peak), its most workgroups with grid = 0, the bases a wavefront covers per step, the multiple to which
 *   a peak's slots are padded, and the most events gx_peak_signal_events takes.  Any pointer may be NULL. */
int gx_peak_signal(gx_ctx* ctx, int* n_samples);
int gx_get_peak_signal(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, int64_t* area120, int64_t* max120, uint32_t* summit,
                       uint32_t* covered, int64_t* at_summit120, size_t cap);
int gx_peak_signal_events(gx_ctx* ctx, const gx_event* ev, size_t n, const gx_region* peaks, size_t n_peaks,
                          const uint32_t* summit_off, unsigned grid, int64_t* area120, int64_t* max120, uint32_t* summit,
                          uint32_t* covered, int64_t* at_summit120);
int gx_peak_signal_geometry(int* lanes, int* grid, uint32_t* step_bases, uint32_t* slot_pad, uint64_t* max_events);

/* ---- sub-summits inside each called peak from the POOLED treatment depth (no Genrich counterpart: a narrowPeak line has one
 *      summit, and a wide peak over two binding sites has two maxima) ----
 * Pooled depth: the sum over all kept TREATMENT samples (controls never) of the depth gx_peak_signal defines: +w at s, -w at
 * the clamped e, w = 120 / count; empty intervals add nothing, intervals with e < s add -w over [e, s); -E regions are not
 * masked.  Per peak [ps, pe) that is d(x), x in [0, L), int64 in 1/120 units.
 * A PLATEAU is a maximal run [a, b) of equal d.  It is a LOCAL MAXIMUM when d is strictly lower on both sides; a side that lies
 * outside the peak counts as lower.  Per local maximum of height h:
 *     pos    = a + (b - a - 1) / 2, the plateau's middle rounded down       width = b - a
 *     prominence = h - max(baseL, baseR); a side's base is the minimum of d over the bases between the plateau and the nearest
 *              base on that side with d > h strictly (none: up to the peak's end); a side whose range is empty (the plateau
 *              touches the peak's edge) is left out of the max; both empty (the plateau is the whole peak): the base is 0.
 *              For interior maxima this is scipy.signal.peak_prominences with wlen=None.
 * Reported: the peak's highest local maximum when h > 0 (of equal maxima the leftmost); every other local maximum with h > 0
 * and  prominence * 100 >= P * h  and  h * 100 >= R * hmax  -- integers, equality keeps the summit; P = prominence_pct, R =
 * height_pct, both 0..100 (the command line's defaults, 25 and 50, are a choice, not a measurement).  A peak whose pooled
 * depth is nowhere positive has no summit.  The summits are ordered by (peak, pos).  Exact integers: no figure depends on the
 * launch geometry, the order of the adds, the push mode or the number of contexts.
 * Domain: a pooled depth below 2^31 (1/120 units) at every base.  Fewer than 2^31 / 120 pooled treatment events cannot leave
 * it; with more, the samples' own maxima per peak are taken first, and a peak in which they add up to 2^31 or more: GX_ERR_ORDER
 * with a text.
 *
 * gx_peak_summits: after gx_find_peaks, with gx_set_count_in_peaks on (else GX_ERR_ORDER); a percentage outside 0..100:
 *   GX_ERR_ORDER with a text.  gx_peak_signal's peak space is cleared once and every kept treatment's k_psig_scatter adds into
 *   it; k_summits (gx_summits.h) gives a wavefront per peak; a peak with more runs than a wavefront's LDS holds is taken by a
 *   second launch with an HBM scratch of the counted size; the summit list is read once more when it ran full.  *n: the
 *   summits.  May be called again, with other percentages; no peak or no treatment is legal (no summit).  Under gx_set_owned a
 *   context handles the peaks of the chromosomes it owns.  gx_get_peak_signal's result stays readable; gx_reset drops this
 *   one.  Its phase is "summits".  Nothing of it is allocated or launched before the first call.
 * gx_get_peak_summits: min(cap, n) summits of the last pass; peak is the index into gx_get_peaks, pos counts from its start.
 * gx_peak_summits_events: the same kernels over n events in host memory, all ONE sample, in n_peaks peaks the caller gives, as
 *   gx_peak_signal_events takes them and with its refusals (GX_ERR_ORDER with a text before anything is allocated or
 *   launched); a percentage above 100 is refused likewise.  grid = 0: the library's geometry, else that many workgroups for
 *   every kernel.  run_cap: the runs a wavefront holds before a peak goes to the second launch (0 or more than the library's:
 *   the library's); list_cap: the list's first capacity (0: the library's).  min(cap, *n_out) summits are written.  It leaves
 *   gx_get_peak_summits' result alone.
 * gx_peak_summits_last: of the last pass of either kind, how often it ran again for a full list (0 or 1) and the peaks its
 *   second launch took.
 * gx_peak_summits_geometry: without a device: the lanes of a workgroup of k_summits (a wavefront of 64 per peak), its most
 *   workgroups with grid = 0, the bases a wavefront covers per step, the runs a wavefront holds, the list's first capacity
 *   max(list_min, list_per_peak * peaks), and the most events gx_peak_summits_events takes.  Any pointer may be NULL. */
typedef struct { uint32_t peak, pos, width, pad; int64_t height120, prominence120; } gx_summit;
int gx_peak_summits(gx_ctx* ctx, int prominence_pct, int height_pct, size_t* n);
int gx_get_peak_summits(gx_ctx* ctx, gx_summit* out, size_t cap);
int gx_peak_summits_events(gx_ctx* ctx, const gx_event* ev, size_t n, const gx_region* peaks, size_t n_peaks, int prominence_pct,
                           int height_pct, unsigned grid, unsigned run_cap, size_t list_cap, gx_summit* out, size_t cap,
                           size_t* n_out);
int gx_peak_summits_last(gx_ctx* ctx, unsigned* reruns, unsigned* big_peaks);
int gx_peak_summits_geometry(int* lanes, int* grid, uint32_t* step_bases, uint32_t* run_cap, uint64_t* list_min,
                             uint32_t* list_per_peak, uint64_t* max_events);

/* ---- binned coverage tracks per sample (no Genrich counterpart: -k, printPile Genrich.c:1697-1715, prints a replicate's pileups
 *      per run-length interval, the control's already scaled and floored; a track wants each sample's own pileup in bins) ----
 * A sample = every gx_sample_end of the run, in call order, as for gx_count_in_peaks: for replicate r its treatment, then its
 * control when one was read; gx_sample_no_control is none.  Its pileup at a base, in 1/120 units (gx_math.h), is what its
 * run-length pileup holds there: the `experimental` column of -k for a treatment (printPile 1697); the control file's own
 * pileup, before factor and lambda, for a control; 0 inside -E regions (-k prints 0.000000 there) and on a chromosome the
 * replicate's treatment header does not list (save[c] == 0) -- after the int16 rule's drops and after every rebuild, because
 * it is read from the pileup the run uses.  With bin size W, chromosome c has ceil(len / W) bins, bin b covers
 * [b W, min((b + 1) W, len)), and sum120[b] is the sum of the pileup over its bases, an exact int64.  Chromosomes that are
 * skipped (-e), empty or not owned by this context (gx_set_owned) have no bins on this context.
 *
 * gx_set_coverage_bins: bin_size 0 = off (default).  Only while idle (after gx_create / gx_reset, before the first
 *   gx_sample_begin) and after gx_set_chroms, else GX_ERR_ORDER; bin_size > 2^20, or more than 2^30 bins in total:
 *   GX_ERR_ORDER.  Survives gx_reset, like gx_set_count_in_peaks.  On, every gx_sample_end runs one more kernel (k_cov_bins,
 *   gx_coverage.h) over the pileup it has just closed and keeps one int64 per bin in device memory until gx_reset (a failed
 *   allocation: GX_ERR_MEM); off, a run launches and allocates nothing for it.
 * gx_coverage_samples: samples closed since the last gx_reset.
 * gx_coverage_bin_count: bins of one chromosome; 0 for a chromosome this context does not compute.
 * gx_coverage_layout: the bin size in effect and the chromosome's length as given to gx_set_chroms (what a formatter needs
 *   besides the sums; either pointer may be NULL).
 * gx_get_coverage: min(cap, n_bins) sums of one sample (0 .. n_samples-1) on one chromosome, its replicate and whether it is a
 *   control (any pointer may be NULL; sum120 when cap is 0).  No sample open, else GX_ERR_ORDER, as for a bad index; it needs
 *   no gx_pvalues and no gx_find_peaks. */
int gx_set_coverage_bins(gx_ctx* ctx, uint32_t bin_size);
int gx_coverage_samples(gx_ctx* ctx, int* n_samples);
int gx_coverage_bin_count(gx_ctx* ctx, int chrom, size_t* n_bins);
int gx_coverage_layout(gx_ctx* ctx, int chrom, uint32_t* bin_size, uint32_t* len);
int gx_get_coverage(gx_ctx* ctx, int sample, int chrom, int* rep, int* is_ctrl, int64_t* sum120, size_t cap);

/* ---- pairwise correlation of the samples from their coverage bins (no Genrich counterpart: the sums deepTools'
 *      multiBamSummary + plotCorrelation take from a second reading of every BAM) ----
 * Samples are 0 .. S-1, the gx_sample_end order of gx_get_coverage.  x_s[b] is sample s's sum120 of bin b over ALL bins of this
 * context: every chromosome that has bins, in table order, the short last bin of a chromosome as it is; bins inside -E regions
 * and of chromosomes a replicate's save mask omits are 0.  With n = the number of bins:
 *     n_zero     = the number of bins b with x_s[b] == 0 for every s
 *     sum[s]     = sum over b of x_s[b]
 *     gram[i][j] = sum over b of x_i[b] x_j[b]              (symmetric; the diagonal is the sum of squares)
 * all exact unsigned 128-bit integers (gx_u128: lo + 2^64 hi).  The bound that makes them exact: x_s[b] <= (2^31 - 1) w_b with
 * w_b <= W the bases of the bin, so a sum of products is at most 2^62 sum w_b^2 <= 2^62 W G, G = the total length of the
 * chromosomes that have bins; the pass is refused (GX_ERR_ORDER) when W G > 2^64, which leaves every sum below 2^126 (hg38 at the
 * largest W = 2^20: W G = 2^52).  Leaving out the all-zero bins changes only n, to n - n_zero: they add nothing to any sum.
 * Everything is an integer: a result does not depend on the grid or on the number of contexts, and a host adds the contexts'
 * n, n_zero, sum and gram (with carries) as it adds region counts; gx_write_correlation_group does.
 *
 * gx_coverage_gram: the pass (k_gram, k_gram_sum: gx_gram.h) over the samples closed since the last gx_reset.  It needs
 *   gx_set_coverage_bins on and at least one closed sample, else GX_ERR_ORDER; also GX_ERR_ORDER: a sample is open, more than
 *   32 samples, the bound above broken, cap < S while sum or gram is given.  sum[cap] and gram[cap * cap] (row-major, row i at
 *   gram + i * cap, both halves filled) may both be NULL: only the counts.  It needs no gx_pvalues and no gx_find_peaks, and may be
 *   called again: the same answer.  A context without bins (it owns no chromosome) answers zeros.  A failed allocation:
 *   GX_ERR_MEM.  Nothing of it is allocated or launched before the first call.
 * gx_gram_u64: the same two kernels over n_rows rows of n values each that the caller gives (host memory, row after row; copied
 *   to the device by this call).  Domain: every value < 2^51, n <= 2^24, 1 <= n_rows <= 32, else GX_ERR_ORDER before anything
 *   is launched.  grid = 0: the library's geometry; else that many workgroups along the bin axis (at most 65535).  n_zero, sum[n_rows] and
 *   gram[n_rows * n_rows] may each be NULL.  For tests and measurements: values and sizes no small pileup produces. */
typedef struct {
  uint64_t lo, hi;
} gx_u128;
int gx_coverage_gram(gx_ctx* ctx, int* n_samples, uint64_t* n_bins, uint64_t* n_zero, gx_u128* sum, gx_u128* gram, int cap);
int gx_gram_u64(gx_ctx* ctx, const uint64_t* rows, int n_rows, size_t n, unsigned grid, uint64_t* n_zero, gx_u128* sum,
                gx_u128* gram);
/* What gx_gram_u64's edge cases depend on: the samples along a tile's edge, the lanes of a workgroup, the most workgroups
 * along the bin axis with grid = 0 (any pointer may be NULL). */
int gx_gram_geometry(int* tile, int* lanes, int* grid);

/* ---- fingerprint (Lorenz curve) of each sample from its coverage bins (no Genrich counterpart: what deepTools'
 *      plotFingerprint takes from another reading of every BAM) ----
 * Samples and x_s[b] are gx_coverage_gram's: all bins of this context, a chromosome's short last bin as it is, 0 inside -E
 * regions and where a replicate's save mask omits the chromosome.  A fingerprint is a function of the distribution of a
 * sample's values only, so the pass reduces every sample to a histogram over value classes.  With M = GX_FP_SUB_LOG = 6:
 *     x < 64:  class(x) = x;     else  e = 63 - clz(x),  class(x) = (e - 6) 64 + (x >> (e - 6))
 * which is continuous and monotone: values below 128 have a class of their own, above that an octave has 64 classes, so a
 * class's values differ by less than 1 / 64 relative; GX_FP_NC = 3776 classes cover uint64 (class(2^64 - 1) = 3775).  The
 * inverse: k < 128: lo(k) = hi(k) = k; else q = k / 64 - 1, lo(k) = (k - 64 q) << q, hi(k) = lo(k) + 2^q - 1.
 *     count[s][k] = the number of bins b with class(x_s[b]) == k
 *     sum[s][k]   = the sum of those x_s[b]
 * both exact uint64.  The bound: x_s[b] <= (2^31 - 1) w_b, so a sample's total is below 2^31 G, G = the total length of the
 * chromosomes that have bins; the pass is refused (GX_ERR_ORDER) when G >= 2^33 (hg38: below 2^32).  A context has at most
 * 2^30 bins, so a count fits 32 bits anywhere on the device.  Integer adds only: a result does not depend on the grid or on
 * the number of contexts, and a host adds the contexts' count and sum class by class (gx_coverage_fingerprint_group does; the
 * bound is then the caller's to keep over all contexts).
 *
 * The curve and the figures are host-only doubles made from those integers (gx_fingerprint_metrics, gx_format_fingerprint).
 * With n = sum_k count[k], T = sum_k sum[k] and C_k, T_k the inclusive running sums, the curve starts at (0, 0) and passes
 * through (p_k, L_k) = (C_k / n, T_k / T) for each non-empty class in ascending order.  These points lie exactly on the
 * sample's Lorenz curve (all bins of a class and below, and all their signal); between two of them the true curve is convex
 * and the polyline lies above it by at most what a spread of 1 / 64 inside one class allows (none below 128).
 *     zero_fraction = count[0] / n            auc  = the polyline's trapezoid sum            gini = 1 - 2 auc
 *     elbow_bins, elbow_gap = p_i and p_i - L_i at the first point where p_i - L_i is largest
 *     jsd_control = for a treatment whose control was read: the square root of the base-2 Jensen-Shannon divergence between
 *                   count_t[k] / n_t and count_c[k] / n_c over the classes; NaN for a control or without one
 * With T == 0 every figure that divides by T is NaN (n == 0: all of them).  Each ratio is one division of integer running
 * sums in long double; auc is added in ascending order in long double.
 *
 * gx_coverage_fingerprint: the pass (k_fp_hist: gx_fingerprint.h) over the samples closed since the last gx_reset.  It needs
 *   gx_set_coverage_bins on and at least one closed sample, else GX_ERR_ORDER; also GX_ERR_ORDER: a sample is open, more than
 *   32 samples, the bound above broken, cap < S while count or sum is given.  count[cap * GX_FP_NC] and sum[cap * GX_FP_NC]
 *   (sample s's row at + s * GX_FP_NC) may each be NULL.  It needs no gx_pvalues and no gx_find_peaks, and may be called
 *   between samples, after them and again: the same answer.  A context without bins answers zeros.  A failed allocation:
 *   GX_ERR_MEM.  Nothing of it is allocated or launched before the first call.
 * gx_fp_u64: the same kernel over n_rows rows of n values each that the caller gives (host memory, row after row; copied to
 *   the device by this call, which adds each row in 128 bits on the way).  Domain: 1 <= n_rows <= 32, n <= 2^24, grid <= 65535,
 *   every row's total below 2^64, else GX_ERR_ORDER before anything is launched; a single value may be anything up to
 *   2^64 - 1.  grid = 0: the library's geometry; else that many workgroups along the bin axis.  count[n_rows * GX_FP_NC] and
 *   sum[n_rows * GX_FP_NC] may each be NULL.  For tests and measurements: values and sizes no small pileup produces.
 * gx_fp_geometry: what gx_fp_u64's edge cases depend on: GX_FP_NC, GX_FP_SUB_LOG, the lanes of a workgroup (each takes two
 *   values a step), the most workgroups of a launch with grid = 0 (with S rows: that divided by S along the bin axis).  Any
 *   pointer may be NULL.
 * gx_fp_class / gx_fp_class_lo / gx_fp_class_hi: class(), lo() and hi() above (host only; lo / hi of k >= GX_FP_NC: 0). */
#define GX_FP_SUB_LOG 6
#define GX_FP_NC ((64 - GX_FP_SUB_LOG + 1) << GX_FP_SUB_LOG)
typedef struct {
  double zero_fraction, auc, gini, elbow_bins, elbow_gap, jsd_control;
} gx_fp_metrics;
int gx_coverage_fingerprint(gx_ctx* ctx, int* n_samples, uint64_t* n_bins, uint64_t* count, uint64_t* sum, int cap);
int gx_fp_u64(gx_ctx* ctx, const uint64_t* rows, int n_rows, size_t n, unsigned grid, uint64_t* count, uint64_t* sum);
int gx_fp_geometry(int* n_classes, int* sub_log, int* lanes, int* grid);
uint32_t gx_fp_class(uint64_t x);
uint64_t gx_fp_class_lo(uint32_t k);
uint64_t gx_fp_class_hi(uint32_t k);

/* ---- Spearman (rank) correlation of the samples from their coverage bins (no Genrich counterpart: what deepTools'
 *      multiBamSummary + plotCorrelation --corMethod spearman take from a second reading of every BAM) ----
 * Samples and x_s[b] are gx_coverage_gram's, over all bins of ALL contexts, a chromosome's short last bin as it is.  Let B be the
 * set of ranked bins: all n of them, or with skip_zeros the n - n_zero bins that are not 0 in every sample (they are taken out
 * BEFORE ranking, as deepTools does: unlike Pearson's sums, the ranks of the bins that stay change).  For a value v of sample s
 *     less_s(v)  = #{b in B : x_s[b] <  v}
 *     equal_s(v) = #{b in B : x_s[b] == v}
 *     R_s[b]     = 2 less_s(x_s[b]) + equal_s(x_s[b]) + 1      for b in B;        R_s[b] = 0 for b outside B
 * R_s[b] is twice the average rank of bin b (ranks counted from 1, ties sharing their mean): an integer, so ties need no
 * fractions, and a correlation does not change when both of its rows are doubled.  A rank is at least 1, so a bin outside B
 * adds nothing to any sum and the Gram pass's own count of all-zero rows counts exactly the bins left out.  Spearman's rho is
 * Pearson's r of the rank rows over B: with N = |B| and sum / gram the exact sums of R over all contexts
 *     rho = gx_correlation_matrix(S, N, 0, sum, gram, 0)
 * Bounds, each refused with GX_ERR_ORDER: at most 32 samples; at most 2^30 bins in a context; N < 2^41 over all contexts, so
 * that R <= 2 N < 2^42 and a sum of products is at most N (2 N)^2 = 4 N^3 < 2^125, inside gx_u128 (4 N^3 < 2^128 needs
 * N < 2^42); N gram < 4 N^4 < 2^166 and sum_i sum_j <= (N (2 N))^2 < 2^166 are inside gx_correlation_matrix's 256-bit
 * differences (they would be up to N < 2^63).  Everything is an integer: a result depends neither on the launch geometry nor
 * on the number of contexts nor on the order in which a table on the device was filled (tables are sorted by value before
 * anything leaves the library).
 *
 * gx_coverage_distinct: one closed sample's distinct bin values over this context's bins, ascending, and how many bins hold
 *   each (k_rank_distinct, k_rank_compact: gx_rank.h).  Order rules: gx_coverage_gram's (coverage bins on, a closed sample, no
 *   sample open, at most 32 samples), a sample index outside the closed samples: GX_ERR_ORDER.  cap = 0: only *n_distinct; else
 *   value[cap] and count[cap] are filled, GX_ERR_ORDER (with *n_distinct set) when cap is too small.  A context without bins: 0.
 * gx_rank_tables: host only, no context.  tables[g * n_samples + s] is context g's table of sample s as gx_coverage_distinct
 *   gives it (strictly ascending values, counts in [1, 2^41)).  Per sample the contexts' tables are merged (equal values add),
 *   n_zero_to_drop is taken off the count of value 0 (0 without skip_zeros; an entry that reaches 0 disappears), and
 *   value[s][k], rank2[s][k] = the merged values ascending and 2 less + equal + 1 of each; n_out[s] = how many.  value and rank2
 *   hold cap entries per sample; both NULL: only n_out and *n_ranked (= N, the same for every sample).  GX_ERR_ORDER: a table
 *   out of order, a count of 0, more to drop than a sample has zeros, samples that differ in N, N >= 2^41, cap too small.
 * gx_coverage_rank_gram: k_rank over this context's bins with the given tables (n_samples of them; value ascending and
 *   never 2^64 - 1, rank2 in [1, 2^42); else GX_ERR_ORDER), then the Gram pass (k_gram, k_gram_sum) over the rank rows: sum and gram as gx_coverage_gram lays them out.
 *   *n_zero = the bins of this context that are 0 in every sample, counted by k_rank itself whether or not they are left out.
 *   A bin's value that is not in its sample's table: GX_ERR_ORDER.  Order rules: gx_coverage_gram's.
 * gx_coverage_spearman_group: the whole pass over the contexts of a run: every context's tables (and with skip_zeros its
 *   all-zero bins, k_rank_nzero), gx_rank_tables, every context's gx_coverage_rank_gram, added with carries.  *n_ranked = N;
 *   n_distinct[n_samples] (may be NULL) = the entries of each sample's merged table.  sum and gram are required.
 * gx_write_spearman_group: that, then gx_format_correlation(out, S, names, N, 0, sum, gram, 0): --correlation's text rules.
 * gx_distinct_u64 / gx_rank_u64: the same kernels over rows the caller gives (host memory; n_rows rows of n values, row after
 *   row; copied to the device by the call).  Domain: every value < 2^51, n <= 2^24, 1 <= n_rows <= 32, grid <= 65535, else
 *   GX_ERR_ORDER before anything is launched.  grid = 0: the library's geometry, else that many workgroups.  gx_rank_u64 ranks
 *   the rows as the samples of one context (rank2[n_rows * n], may be NULL) and gives the all-zero bins in *n_zero.
 * gx_rank_geometry: what their edge cases depend on: the lanes of a workgroup of k_rank_distinct (each takes two values a
 *   step), the most workgroups with grid = 0, the entries of a workgroup's LDS cache, the table's first capacity and the most
 *   distinct non-zero values it takes before it grows (the same half of every capacity).  Any pointer may be NULL.
 * gx_rank_last: the capacity the last k_rank_distinct pass of this context ended with (0: none yet) and how often it grew.
 * Nothing of all this is allocated or launched before the first call. */
typedef struct {
  const uint64_t* value;   /* ascending */
  const uint64_t* count;
  size_t n;
} gx_rank_table;
typedef struct {
  const uint64_t* value;   /* ascending */
  const uint64_t* rank2;
  size_t n;
} gx_rank_lut;
int gx_coverage_distinct(gx_ctx* ctx, int sample, uint64_t* value, uint64_t* count, size_t cap, size_t* n_distinct);
int gx_rank_tables(int n_ctx, int n_samples, const gx_rank_table* tables, uint64_t n_zero_to_drop, uint64_t* const* value,
                   uint64_t* const* rank2, size_t cap, size_t* n_out, uint64_t* n_ranked);
int gx_coverage_rank_gram(gx_ctx* ctx, const gx_rank_lut* tables, int skip_zeros, int* n_samples, uint64_t* n_bins, uint64_t* n_zero,
                          gx_u128* sum, gx_u128* gram, int cap);
int gx_coverage_spearman_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, int skip_zeros, uint64_t* n_ranked, gx_u128* sum,
                               gx_u128* gram, uint64_t* n_distinct);
int gx_distinct_u64(gx_ctx* ctx, const uint64_t* row, size_t n, unsigned grid, uint64_t* value, uint64_t* count, size_t cap,
                    size_t* n_distinct);
int gx_rank_u64(gx_ctx* ctx, const uint64_t* rows, int n_rows, size_t n, unsigned grid, int skip_zeros, uint64_t* rank2,
                uint64_t* n_zero);
int gx_rank_geometry(int* lanes, int* grid, int* cache_entries, size_t* first_capacity, size_t* load_limit);
int gx_rank_last(gx_ctx* ctx, size_t* capacity, int* n_grown);

/* ---- library complexity of each sample's intervals (no Genrich counterpart: NRF, PBC1, PBC2, Picard's estimated library size
 *      and preseq's c_curve, which otherwise want the whole BAM sorted into a bedpe, or another reading of it) ----
 * A sample = every gx_sample_end of the run in call order, as for gx_count_in_peaks.  Its intervals are exactly those
 * gx_count_in_peaks counts, i.e. its -b lines: count valid (1-6, 8 or 10), chromosome known, not skipped (-e), in the
 * sample's save mask and owned by this context, start < the chromosome's length, the end clamped to that length; empty
 * intervals are included, and so are intervals that end before they start, as they are.  Each interval is ONE observation,
 * whatever its -s weight.  Its key is the triple (chrom, start, clamped end); `count` is not part of it.  Two ends that differ
 * but clamp to the same length are the same key; the same coordinates on two chromosomes are two keys.  Per sample, all
 * exact uint64:
 *     N    = observations          D = distinct keys          h[m] = the number of keys seen exactly m times
 * so that sum h[m] = D and sum m h[m] = N.  h is reported sparse: (m, h[m]) pairs with h[m] > 0, ascending in m.  A key lives
 * on one chromosome and a chromosome on one context, so the contexts' N, D and h simply add (gx_complexity_group does).  The
 * result is the same for every launch geometry, table capacity, push mode and number of GPUs: integer adds only.
 * In -j ATAC mode a fragment contributes its two cut-site intervals, and the figures are over cut sites, not fragments.  After
 * -r the figures describe what -r left (its duplicates never reach the library).  Events carry no strand: none in the key.
 * Limits, each refused with GX_ERR_ORDER and a text before anything is allocated or launched: the device's key is 64 bits,
 * 32 of them the start in the context's tile space (every chromosome's length rounded up to a tile, added), so that space
 * must not exceed 2^32 - 1 bases (hg38: 3.1 * 10^9); a sample of 2^31 events or more on one context.
 *
 * gx_complexity: the pass (k_cpx_insert, k_cpx_hist: gx_complexity.h) over every sample closed so far (*n_samples of them): per
 *   sample a table of at least 2 n slots for its n events, sized once and reused for the next sample.  It needs
 *   gx_set_count_in_peaks on, at least one closed sample and none open, else GX_ERR_ORDER with a text; it needs no gx_pvalues
 *   and no gx_find_peaks, and may be called again: the same answer.  The results of gx_count_in_peaks / gx_count_in_regions
 *   stay readable.  gx_reset drops the result.  A failed allocation: GX_ERR_MEM.  A bounded loop of the kernels that ran out
 *   (it cannot, with a table at most half full): GX_ERR_DEVICE with a text, never a hang.  Nothing of it is allocated or
 *   launched before the first call.
 * gx_get_complexity: the last pass's result for one sample (0 .. n_samples-1): its replicate, whether it is a control, N, D,
 *   min(cap, n_classes) pairs in mult[] / keys[] and *n_classes.  Any pointer may be NULL (mult and keys when cap is 0).
 * gx_complexity_events: the same two kernels over n events in host memory (copied to the device by the call), all treated as
 *   ONE sample whose save mask lists every chromosome of the context's table (-e and gx_set_owned hold as for a sample).
 *   grid = 0 and cap_log = 0: the library's choices; else that many workgroups (at most 65535) for either kernel and a table of
 *   2^cap_log slots; 2^cap_log < 2 n (or cap_log > 32): GX_ERR_ORDER before anything is launched.  No sample open.  For tests
 *   and measurements; it leaves gx_get_complexity's result alone.
 * gx_complexity_geometry: what the edge cases depend on: the lanes of a workgroup of k_cpx_insert, its most workgroups with
 *   grid = 0, the bound below which k_cpx_hist counts a multiplicity in LDS (at or above it the key goes to a list), and the
 *   least capacity for n events (0: n >= 2^31).  Any pointer may be NULL.  gx_complexity_last: the capacity the last pass used.
 * gx_complexity_group: sample `sample` of every context's last gx_complexity, added; the outputs as gx_get_complexity's.  A
 *   context without a result, or contexts that differ in their samples: GX_ERR_ORDER. */
int gx_complexity(gx_ctx* ctx, int* n_samples);
int gx_get_complexity(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, uint64_t* n_obs, uint64_t* n_distinct, uint64_t* mult,
                      uint64_t* keys, size_t cap, size_t* n_classes);
int gx_complexity_events(gx_ctx* ctx, const gx_event* ev, size_t n, unsigned grid, int cap_log, uint64_t* n_obs,
                         uint64_t* n_distinct, uint64_t* mult, uint64_t* keys, size_t cap, size_t* n_classes);
int gx_complexity_geometry(int* lanes, int* grid, uint32_t* lds_bound, uint64_t n, size_t* least_capacity);
int gx_complexity_last(gx_ctx* ctx, size_t* capacity);
int gx_complexity_group(gx_ctx* const* ctxs, int n_ctx, int sample, int* rep, int* is_ctrl, uint64_t* n_obs, uint64_t* n_distinct,
                        uint64_t* mult, uint64_t* keys, size_t cap, size_t* n_classes);

/* ---- lengths and per-chromosome tallies of each sample's intervals (no Genrich counterpart: the fragment-length distribution
 *      of deepTools' bamPEFragmentSize or Picard's CollectInsertSizeMetrics, and `samtools idxstats`, which otherwise want
 *      another reading of the BAM) ----
 * A sample = every gx_sample_end of the run in call order, as for gx_count_in_peaks.  Its intervals are exactly those
 * gx_count_in_peaks counts, i.e. its -b lines (the rule is gx_complexity's, above): count valid, chromosome known, not skipped
 * (-e), in the sample's save mask and owned by this context, start < the chromosome's length, the end clamped to that length;
 * empty intervals are included.  An interval whose clamped end lies below its start is INVERTED and has no length; every other
 * has the length L = end - start >= 0.  Its weight is w = 120 / count, in 1/120 units.  Per sample, all exact uint64:
 *     n[L], w120[L]             the intervals of length L and their summed weight, for every L that occurs
 *     n_inverted, w120_inverted the inverted intervals: counted only here and in cn / cw120
 *     cn[c], cw120[c]           the intervals on chromosome c of the table and their weight
 *     cbases120[c]              sum of w L over the intervals on c that have a length: 120 x the bases they cover, with multiplicity
 * so that sum n[L] + n_inverted = sum cn[c], the same for the weights, and sum w120[L] L = sum cbases120[c]: the host checks
 * the three after every pass (GX_ERR_DEVICE with a text when one fails).  A chromosome lives on one context, so the contexts'
 * results simply add (gx_interval_stats_group does).  The result is the same for every launch geometry, list capacity, push
 * mode and number of GPUs: integer adds only.  A chromosome skipped with -e never reaches the library: its tallies are zeros.
 * In -j ATAC mode the intervals are cut-site windows, two per fragment and nearly all of one length: the figures describe
 * those windows, not fragments.
 * Limits, each refused with GX_ERR_ORDER and a text before anything is allocated or launched: a sample of 2^31 events or
 * more on one context; more than 65535 workgroups; a grid that lets a workgroup see more than 272 chunks of 65536 events
 * (its LDS counters are 32 bits).
 *
 * gx_interval_stats: the pass (k_ivstat, gx_ivstat.h) over every sample closed so far (*n_samples of them).  It needs
 *   gx_set_count_in_peaks on, at least one closed sample and none open, else GX_ERR_ORDER with a text; it needs no gx_pvalues
 *   and no gx_find_peaks, and may be called again: the same answer.  The results of gx_count_in_peaks, gx_count_in_regions and
 *   gx_complexity stay readable.  gx_reset drops the result.  A failed allocation: GX_ERR_MEM.  Lengths of GX_IVS_BOUND or
 *   more go through a list in device memory; when it runs full the sample is run once more with a list of the counted size,
 *   exactly once.  Nothing of it is allocated or launched before the first call.
 * gx_get_interval_lengths: the last pass's result for one sample (0 .. n_samples-1): its replicate, whether it is a control,
 *   min(cap, n_classes) entries in length[] / n[] / w120[] ascending in the length, *n_classes and the inverted ones.  Any
 *   pointer may be NULL (the arrays when cap is 0).
 * gx_get_chrom_stats: min(cap, chromosomes) entries per array, in table order.
 * gx_interval_stats_events: the same kernel over n events in host memory (copied to the device by the call), all treated as ONE
 *   sample whose save mask lists every chromosome of the context's table (-e and gx_set_owned hold as for a sample).  grid = 0
 *   and list_cap = 0: the library's choices; else that many workgroups and a list of that many entries at first.  No sample
 *   open.  For tests and measurements; it leaves the kept result alone.
 * gx_interval_stats_geometry: what the edge cases depend on: the lanes of a workgroup, the most workgroups with grid = 0 (more
 *   only when a sample has more than 272 chunks per workgroup), the length from which an interval goes to the list, the
 *   chromosomes tallied in LDS (the others by global atomics), and the list's first capacity.  Any pointer may be NULL.
 * gx_interval_stats_last: the list capacity the last pass ended with and how often it ran again (0 or 1).
 * gx_interval_stats_group: sample `sample` of every context's last gx_interval_stats, added; the outputs as the two getters'.
 *   A context without a result, or contexts that differ in their samples: GX_ERR_ORDER. */
#define GX_IVS_BOUND 4096
int gx_interval_stats(gx_ctx* ctx, int* n_samples);
int gx_get_interval_lengths(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, uint64_t* length, uint64_t* n, uint64_t* w120, size_t cap,
                            size_t* n_classes, uint64_t* n_inverted, uint64_t* w120_inverted);
int gx_get_chrom_stats(gx_ctx* ctx, int sample, uint64_t* cn, uint64_t* cw120, uint64_t* cbases120, size_t cap);
int gx_interval_stats_events(gx_ctx* ctx, const gx_event* ev, size_t n, unsigned grid, size_t list_cap, uint64_t* length, uint64_t* n_iv,
                             uint64_t* w120, size_t cap, size_t* n_classes, uint64_t* n_inverted, uint64_t* w120_inverted, uint64_t* cn,
                             uint64_t* cw120, uint64_t* cbases120, size_t chrom_cap);
int gx_interval_stats_geometry(int* lanes, int* grid, uint32_t* lds_bound, uint32_t* chrom_window, size_t* list_capacity);
int gx_interval_stats_last(gx_ctx* ctx, size_t* list_capacity, int* reruns);
int gx_interval_stats_group(gx_ctx* const* ctxs, int n_ctx, int sample, int* rep, int* is_ctrl, uint64_t* length, uint64_t* n, uint64_t* w120,
                            size_t cap, size_t* n_classes, uint64_t* n_inverted, uint64_t* w120_inverted, uint64_t* cn, uint64_t* cw120,
                            uint64_t* cbases120, size_t chrom_cap);

/* ---- strand cross-correlation of each sample's 5' ends (no Genrich counterpart: the curve and the three figures -- estimated
 *      fragment length, NSC, RSC -- of phantompeakqualtools / SPP, MACS2 predictd or Q, which ENCODE asks of every ChIP-seq library
 *      and which otherwise want another tool and another reading of the BAM; for a single-end library the fragment length is
 *      also what -y's -x N should be) ----
 * TAGS.  A tag is (chromosome, position, strand) of an alignment's 5' end, taken from the alignment's own coordinates: a forward
 * alignment gives (+, first aligned base), a reverse one (-, last aligned base), a properly paired fragment both (+, its first
 * base) and (-, its last base).  The caller makes them (the command line does, where an alignment becomes intervals, before -j /
 * -y / -x / -w / -d / -D and the clamping change those) and pushes them beside the sample's events.  The library keeps two bit
 * vectors per open sample, one per strand, one bit per base: a position tagged twice is tagged once, weights do not exist.  A tag
 * on a chromosome that is skipped (-e), outside the sample's save mask or not owned by the context sets nothing; -E regions are
 * not masked.  A tag whose chromosome lies beyond the table, whose position lies at or beyond the chromosome's length or whose
 * strand is neither 0 nor 1 sets nothing and is counted in `rejected`.
 * COUNTS, per sample, all exact uint64:
 *     n_pos            N, the summed lengths of the chromosomes that take part (saved, not skipped, owned)
 *     n_plus, n_minus  the set bits of the two vectors
 *     n11[d - lo]      for every shift lo <= d <= hi: the positions (c, x) with plus_c[x] and minus_c[x + d], 0 <= x, x + d < len_c;
 *                      pairs never cross a chromosome's border; d may be negative
 * They are the same for every launch geometry, order and split of the tags and number of GPUs (a chromosome lives on one
 * context: the contexts' counts add, gx_xcor_group).
 * CURVE (host, gx_xcor_metrics):  r(d) = (N n11(d) - n_plus n_minus) / sqrt(n_plus (N - n_plus) n_minus (N - n_minus)), numerator
 * and radicand exact (128 / 256 bits), each converted once; NaN ("NA") when the radicand is 0.  r uses the UNSHIFTED totals: a
 * Pearson coefficient over the overlap of the two shifted windows differs from it by O(d / len).  This is the definition here.
 * LAYOUT AND LIMITS.  Every chromosome starts on a 64-bit word; before and after each lie ceil(max(|lo|, |hi|) / 64) + 1 zero
 * words, so a shifted window never reads another chromosome's bits.  Two vectors of (genome / 8) bytes per context: 2 x 388 MB
 * for hg38.  Refused with GX_ERR_ORDER and a text: shifts outside -GX_XCOR_MAX_SHIFT <= lo <= hi <= GX_XCOR_MAX_SHIFT; a genome
 * of 2^37 bases or more.  A failed allocation: GX_ERR_MEM.
 *
 * gx_set_xcor: on, with the shifts lo .. hi; hi < lo: off, the vectors are freed.  After gx_set_chroms, on an idle context before
 *   its first sample (else GX_ERR_ORDER); the vectors are allocated here (and again when gx_set_chroms / gx_set_owned change the
 *   table).  They are cleared at every gx_sample_begin, and gx_sample_end makes the pass (k_xc_corr, gx_xcor.h) and keeps the
 *   sample's counts on the host.  gx_reset drops the results and keeps the setting.  Off: nothing is allocated, launched or recorded.
 * gx_push_tags: n tags of the open sample, in any order and any split (k_xc_set: one 64-bit atomic OR per tag); the caller's
 *   memory is free on return.  Without gx_set_xcor, or with no sample open: GX_ERR_ORDER.
 * gx_xcor_samples / gx_get_xcor: the samples closed since gx_set_xcor / gx_reset, in call order; min(cap, hi - lo + 1) entries
 *   of n11.  Any pointer may be NULL (n11 when cap is 0).
 * gx_xcor_group: sample `sample` of every context, added.  Contexts that differ in their samples or shifts: GX_ERR_ORDER.
 * gx_xcor_tags: the two kernels alone over n tags in host memory and a table of n_chrom lengths of its own, every chromosome
 *   taking part: vectors of its own, released on return; the context's setting and results are left alone.  grid = 0 /
 *   tile_words = 0: the library's choices; else that many workgroups (at most 65535) and plus words per tile (a multiple of
 *   GX_XCOR_MIN_TILE from there to the default).  No sample open.  For tests and measurements.
 * gx_xcor_geometry: the lanes of a workgroup of k_xc_corr, its most workgroups with grid = 0, the default words per tile, the
 *   padding words of the widest setting, and the plus words a workgroup walks at most before it adds its 32-bit counters to the
 *   64-bit ones (2^25: 2^25 words x 64 pairs < 2^32).  Any pointer may be NULL. */
#define GX_XCOR_MAX_SHIFT 4096
#define GX_XCOR_MIN_TILE 64
typedef struct { uint32_t chrom; uint32_t pos; uint32_t strand; /* 1: +, 0: - */ } gx_tag;
int gx_set_xcor(gx_ctx* ctx, int lo, int hi);
int gx_push_tags(gx_ctx* ctx, const gx_tag* tags, size_t n);
int gx_xcor_samples(gx_ctx* ctx, int* n_samples);
int gx_get_xcor(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, uint64_t* n_pos, uint64_t* n_plus, uint64_t* n_minus, uint64_t* rejected, int* lo,
                int* hi, uint64_t* n11, size_t cap);
int gx_xcor_group(gx_ctx* const* ctxs, int n_ctx, int sample, int* rep, int* is_ctrl, uint64_t* n_pos, uint64_t* n_plus, uint64_t* n_minus,
                  uint64_t* rejected, int* lo, int* hi, uint64_t* n11, size_t cap);
int gx_xcor_tags(gx_ctx* ctx, const uint32_t* lens, int n_chrom, const gx_tag* tags, size_t n, int lo, int hi, unsigned grid, uint32_t tile_words,
                 uint64_t* n_pos, uint64_t* n_plus, uint64_t* n_minus, uint64_t* rejected, uint64_t* n11, size_t cap);
int gx_xcor_geometry(int* lanes, int* grid, uint32_t* tile_words, uint32_t* pad_words_for_4096, uint64_t* flush_words);

/* ---- the reference sequence, GC bias per sample and GC content per interval (no Genrich counterpart: deepTools' computeGCBias,
 *      the fragment model of Benjamini & Speed, which otherwise wants another tool and another reading of the BAM and the
 *      genome) ----
 * THE GENOME, per context: two bit vectors, one bit per base.  gc has bit x set when base x is one of G C g c, acgt when it is
 * one of A C G T a c g t.  Everything else is UNKNOWN: N, IUPAC codes, bases never pushed, positions past a chromosome's end.
 * THE WINDOW of width W (1 .. GX_GC_MAX_WINDOW) at position x of a chromosome is [x, x + W).  It is CLASSED iff all W of its
 * acgt bits are set; its class is then g, its gc bits, 0 <= g <= W.
 * COUNTS, per sample, all exact uint64:
 *     F[g]             the classed windows over all positions of the chromosomes that take part (saved, not skipped, owned);
 *     f_unclassed      ... the positions of those chromosomes whose window is not classed
 *     Nn[g], Nw[g]     the sample's intervals (exactly its -b lines, gx_set_count_in_peaks) whose window AT THE INTERVAL'S START
 *                      is classed g, and their weight in 1/120 units; the interval's own length plays no part (deepTools'
 *                      construction), so cut-site windows and inverted intervals count like the rest
 *     n_unclassed, w_unclassed   the intervals whose window is not classed, and their weight
 * -E regions are NOT masked on either side (as for gx_peak_signal).  The counts are the same for every launch geometry, split
 * of the pushes and number of GPUs (a chromosome lives on one context: the contexts' counts add, gx_gc_bias_group).
 * FIGURES (host, gx_gc_metrics): the classes folded into GX_GC_CLASSES percent classes, k = (200 g + W) / (2 W) in integers
 * (halves up); ratio[k] = (Nw[k] / sum Nw) / (F[k] / sum F) = double(Nw[k] * sum F) / double(F[k] * sum Nw), both products exact
 * 128-bit integers, each converted once (the leading 64 bits, then one rounding, as for gx_xcor_r); NaN ("NA") where F[k] or
 * sum Nw is 0.
 * LAYOUT AND LIMITS.  Every chromosome starts on a 512-base block; before and after each lie at least GX_GC_MAX_WINDOW / 64 + 1
 * zero words.  Two vectors of (genome / 8) bytes and a rank directory of (genome / 64) bytes per context: 2 x 388 MB + 48 MB for
 * hg38.  Refused with GX_ERR_ORDER and a text: a window outside 1 .. GX_GC_MAX_WINDOW; a genome of 2^37 bases or more.
 *
 * gx_set_genome: on != 0: the vectors for the context's table are allocated and cleared (every base unknown); 0: freed.  After
 *   gx_set_chroms, with no sample open.  gx_set_chroms / gx_set_owned lay the vectors out again, EMPTY: the bases are pushed
 *   again.  gx_reset keeps the genome and drops gx_gc_bias' results.  Off: nothing is allocated, launched or recorded.
 * gx_push_sequence: n plain sequence bytes (no newlines) of chromosome chrom from base first_base on; any order, any split, at
 *   any time; the caller's memory is free on return.  first_base must be a multiple of 64, and only a chromosome's last push
 *   (first_base + n = its length) may have n % 64 != 0: every word has one writer.  The same stretch pushed twice is harmless.
 *   GX_ERR_ORDER with a text: a chromosome outside the table, bases past its length, a first_base or an n that breaks the rule.
 *   A chromosome that is skipped or not owned takes nothing, with no error, as tags do.
 * gx_genome_info: the bases pushed (per chromosome the end of its furthest push, added) and the set bits of both vectors.
 * gx_gc_content: for n intervals, the gc and the acgt bits in [start, min(end, length)); end <= start, a chromosome outside the
 *   table or without words here: 0.
 * gx_gc_bias: the tables of every closed kept sample (needs gx_set_count_in_peaks' keeping, no sample open, no peaks).  F is
 *   computed once per distinct set of chromosomes among the samples (k_gc_expected), Nn / Nw by one pass per sample
 *   (k_gc_observed).  gx_get_gc_bias: sample `sample` of the last gx_gc_bias, min(cap, W + 1) classes of each table; any
 *   pointer may be NULL (the tables when cap is 0).  gx_gc_bias_group: that sample of every context, added.
 * gx_gc_bias_events: the same kernels over the context's genome and n events in host memory (packed != 0: gx_event8 records),
 *   taken as ONE sample that saves every chromosome.  grid_expected / tile_words / flush_words / grid_observed = 0: the
 *   library's choices; else that many workgroups (at most 65535), words per tile of k_gc_expected (a multiple of
 *   GX_GC_MIN_TILE from there to 1024) and words a workgroup of it walks at most between two flushes of its 32-bit counters
 *   (from one tile to 2^25).  No sample open.  For tests and measurements.
 * gx_gc_geometry: the lanes of a workgroup of k_gc_expected, its most workgroups with grid = 0, its default and smallest words
 *   per tile, the zero words around a chromosome, the bases per directory block, and the flush bound (2^25 words x 64 windows
 *   < 2^32).  Any pointer may be NULL. */
#define GX_GC_MAX_WINDOW 4096
#define GX_GC_MIN_TILE 64
#define GX_GC_CLASSES 101
int gx_set_genome(gx_ctx* ctx, int on);
int gx_push_sequence(gx_ctx* ctx, int chrom, uint64_t first_base, const char* bases, size_t n);
int gx_genome_info(gx_ctx* ctx, uint64_t* bases_pushed, uint64_t* gc, uint64_t* acgt);
int gx_gc_content(gx_ctx* ctx, const gx_region* regions, size_t n, uint64_t* gc, uint64_t* acgt);
int gx_gc_bias(gx_ctx* ctx, int window, int* n_samples);
int gx_get_gc_bias(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, int* window, uint64_t* F, uint64_t* f_unclassed, uint64_t* Nn, uint64_t* Nw,
                   uint64_t* n_unclassed, uint64_t* w_unclassed, size_t cap);
int gx_gc_bias_group(gx_ctx* const* ctxs, int n_ctx, int sample, int* rep, int* is_ctrl, int* window, uint64_t* F, uint64_t* f_unclassed, uint64_t* Nn,
                     uint64_t* Nw, uint64_t* n_unclassed, uint64_t* w_unclassed, size_t cap);
int gx_gc_bias_events(gx_ctx* ctx, const void* ev, size_t n, int packed, int window, unsigned grid_expected, uint32_t tile_words, uint64_t flush_words,
                      unsigned grid_observed, uint64_t* F, uint64_t* f_unclassed, uint64_t* Nn, uint64_t* Nw, uint64_t* n_unclassed,
                      uint64_t* w_unclassed, size_t cap);
int gx_gc_geometry(int* lanes, int* grid, uint32_t* tile_words, uint32_t* min_tile_words, uint32_t* pad_words, uint32_t* block_bases,
                   uint64_t* flush_words);
/* The figures and the tables (host only, gx_emit.cpp).  gx_gc_class: the percent class of g in a window of W (-1: out of range).
 * gx_gc_metrics: the folded tables, the ratios, the mean window GC of the genome (sum g F[g] / (W sum F)) and of the sample's
 * intervals (weighted: sum g Nw[g] / (W sum Nw)), and the least and the greatest ratio among the classes that hold at least 1 %
 * of the classed windows (class -1 and NaN: none).  GX_ERR_ORDER: a table that contradicts itself (a weight outside
 * Nn <= Nw <= 120 Nn).  gx_format_gc_bias: --gc-bias' table: a header, then per sample one `#` line (W, the classed and the
 * unclassed windows and intervals) and GX_GC_CLASSES rows `sample gc_percent windows intervals weight ratio`; weights as --counts
 * prints a count.  gx_format_gc_peaks: --gc-peaks' table: the rows of --counts (chr start end peak_N, in the order given), then
 * length, acgt, gc and gc / acgt ("NA" when acgt is 0).  gx_write_gc_bias_group: gx_gc_bias on every context, the sums, the
 * table.  gx_write_gc_peaks_group: gx_gc_content on every context's own peaks, the table of the merged peaks (see
 * gx_write_narrowpeak_group). */
typedef struct {
  uint64_t windows, windows_unclassed, intervals, intervals_unclassed, w120, w120_unclassed;
  uint64_t cls_windows[GX_GC_CLASSES], cls_intervals[GX_GC_CLASSES], cls_w120[GX_GC_CLASSES];
  double ratio[GX_GC_CLASSES];
  double mean_gc_genome, mean_gc_sample, ratio_min, ratio_max;
  int32_t ratio_min_class, ratio_max_class;
} gx_gc_metrics_t;
int gx_gc_class(int window, int g);
int gx_gc_metrics(int window, const uint64_t* F, uint64_t f_unclassed, const uint64_t* Nn, const uint64_t* Nw, uint64_t n_unclassed,
                  uint64_t w_unclassed, gx_gc_metrics_t* out);
int gx_format_gc_bias(FILE* out, int n_samples, const int* rep, const int* is_ctrl, int window, const uint64_t* const* F, const uint64_t* f_unclassed,
                      const uint64_t* const* Nn, const uint64_t* const* Nw, const uint64_t* n_unclassed, const uint64_t* w_unclassed);
int gx_format_gc_peaks(FILE* out, const char* const* names, const gx_region* peaks, size_t n_peaks, const uint64_t* gc, const uint64_t* acgt);
int gx_write_gc_peaks_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, FILE* out);
int gx_write_gc_bias_group(gx_ctx* const* ctxs, int n_ctx, int window, FILE* out);

/* ---- the sequence itself and known motifs scanned in the called peaks and in the genome (no Genrich counterpart: what HOMER's
 *      findMotifsGenome -find, FIMO or MOODS do with the peak sequences cut out of the FASTA once more) ----
 * THE SEQUENCE, per context: a third bit vector `ag` with the layout, the padding and the one-writer-per-word rule of gc and
 * acgt; its bit is set for A G a g.  With gc it names a known base (acgt = 1): A = (gc 0, ag 1), C = (1, 0), G = (1, 1),
 * T = (0, 0); the complement is the base with the ag bit flipped; a base whose acgt bit is 0 stays unknown.
 * A MOTIF has a width L, 1 <= L <= GX_MOTIF_MAX_WIDTH, an L x 4 table of int16 scores s[j][b] in column order A C G T and an
 * int32 threshold t; a context takes at most GX_MOTIF_MAX of them.
 * THE WINDOW of motif m at position x of a region [start, end) on chromosome c is [x, x + L).  It is SCANNED iff start <= x,
 * x + L <= min(end, len[c]) and all L of its acgt bits are set.  Its forward score is sum_j s[j][base(x + j)], its reverse score
 * sum_j s[j][comp(base(x + L - 1 - j))].  A HIT is a scanned window and a strand whose score is >= t: both strands may hit at one
 * x (a palindrome then reports two).
 * COUNTS per motif, all exact uint64: windows (scanned), hits_fwd, hits_rev.  Over a set of regions every region is scanned on
 * its own (overlapping regions count twice); over the genome the counts run over every chromosome that takes part (not
 * skipped, owned, and saved by the last treatment sample begun; before any sample: every one), and add over contexts.
 * THE HIT LIST: gx_motif_hit records; pos counts from the region's start; sorted by (region, pos, motif, strand).  -E regions
 * are NOT masked (as for gx_peak_signal and gx_gc_bias).  No result depends on the launch geometry, the step, the motif batch,
 * the list's capacity, the split of the pushes or the number of GPUs.
 *
 * gx_set_genome_bases: on != 0: after gx_set_genome(ctx, 1) and before any base is pushed (else GX_ERR_ORDER with a text): ag
 *   is allocated and cleared, and from then on gx_push_sequence fills all three vectors (k_seq_pack3).  Off (the default):
 *   nothing more is allocated and the pushes launch k_gc_pack as before.  gx_set_chroms / gx_set_owned lay ag out again, empty,
 *   with the other two; gx_reset keeps it; gx_set_genome(ctx, 0) frees it.  gx_genome_info, gx_gc_content and gx_gc_bias* give
 *   the same results with the bases on.
 * gx_get_sequence: n letters of chromosome chrom from base start on (k_seq_unpack): upper-case A C G T, N for an unknown base
 *   and for every position past the chromosome's end or on a chromosome without words here.  out holds n bytes (no terminator).
 * gx_set_motifs: n motifs; motif i's table is the 4 * width int16 at scores + m[i].offset (row j: s[j][A], s[j][C], s[j][G],
 *   s[j][T]).  A width outside 1 .. GX_MOTIF_MAX_WIDTH or more than GX_MOTIF_MAX motifs: GX_ERR_ORDER with a text.  n = 0 drops
 *   them.  The results of the last gx_motif_scan_peaks go with the old motifs.
 * gx_motif_scan_regions: k_motif_scan over n regions of the caller's (any order, overlapping, empty or inverted; a chromosome
 *   outside the table or without words here scans nothing).  Needs the bases; no sample, no events and no peaks.  grid /
 *   step_words / batch_motifs / list_cap = 0: the library's choices; else that many workgroups (at most 65535, and enough
 *   that none walks more than the flush bound: gx_motif_grid), runs of 64 positions a wavefront takes per unit of work (1 .. 16), motifs per
 *   LDS batch (1 .. 64) and entries of the first hit list (below 2^31; 0: one entry per 2048 positions of the regions and
 *   motif, at least the geometry's least capacity and at most 2^24).  The list is counted: when it ran full the pass is run
 *   once more with a list of the counted size; 2^31 hits or more are refused with a text.  out takes min(cap, *n_out) hits;
 *   windows / hits_fwd / hits_rev take one count per motif set (NULL: not wanted; all three or none).  For tests and
 *   measurements.
 * gx_motif_scan_peaks: after gx_find_peaks, with no sample open, the bases on and motifs set (else GX_ERR_ORDER): the peaks
 *   this context called are the regions (region = the peak's index in gx_get_peaks).  No peak or no motif is legal.  Nothing of
 *   it is allocated or launched before the first call; its phase is "motifs".  gx_get_motif_hits: min(cap, *n_hits) of them;
 *   gx_get_motif_counts: min(cap, motifs) of each count.  Until gx_reset, gx_set_motifs or the next sample.
 * gx_motif_last: how often the last scan ran again (0 or 1) and its LDS batches.
 * gx_motif_scan_genome: the count-only instance over every chromosome that takes part; min(cap, motifs) of each count.
 *   gx_motif_scan_genome_group: the contexts' counts added (a chromosome lives on one context).
 * gx_motif_geometry: the lanes of a workgroup of k_motif_scan, its most workgroups with grid = 0, the positions a wavefront
 *   takes per step (64), the default runs per unit, the motifs per LDS batch, the first list's least capacity and the flush
 *   bound: the runs a WORKGROUP walks at most per batch (its four wavefronts add to the same 32-bit LDS counters, at most 64 per
 *   run: 2^25 x 64 = 2^31 < 2^32).  Any pointer may be NULL.  No device.
 * gx_motif_grid: the grid a pass over `units` units of step_words runs (0: the default) takes: with grid = 0 the library's
 *   choice in *chosen, else the caller's, or GX_ERR_ORDER when it is refused -- a step outside 1 .. 16, more than 65535
 *   workgroups, 2^32 units or more, or a grid so small that a workgroup would walk more than the flush bound: a workgroup takes
 *   four units per round, so it needs grid >= ceil(ceil(units / 4) / (2^25 / (4 step_words))).  No device, no context. */
#define GX_MOTIF_MAX_WIDTH 32
#define GX_MOTIF_MAX 4096
#define GX_MOTIF_SCALE 128
typedef struct { uint32_t width, offset; int32_t threshold; } gx_motif;
typedef struct { uint32_t region, pos; int32_t score; uint16_t motif; uint8_t strand /* 0 +, 1 - */, pad; } gx_motif_hit;
int gx_set_genome_bases(gx_ctx* ctx, int on);
int gx_get_sequence(gx_ctx* ctx, int chrom, uint64_t start, size_t n, char* out);
int gx_set_motifs(gx_ctx* ctx, const gx_motif* m, int n, const int16_t* scores);
int gx_motif_scan_regions(gx_ctx* ctx, const gx_region* regions, size_t n, unsigned grid, uint32_t step_words, uint32_t batch_motifs, size_t list_cap,
                          gx_motif_hit* out, size_t cap, size_t* n_out, uint64_t* windows, uint64_t* hits_fwd, uint64_t* hits_rev);
int gx_motif_scan_peaks(gx_ctx* ctx, size_t* n_hits);
int gx_get_motif_hits(gx_ctx* ctx, gx_motif_hit* out, size_t cap);
int gx_get_motif_counts(gx_ctx* ctx, uint64_t* windows, uint64_t* hits_fwd, uint64_t* hits_rev, size_t cap);
int gx_motif_last(gx_ctx* ctx, uint32_t* reruns, uint32_t* batches);
int gx_motif_scan_genome(gx_ctx* ctx, uint64_t* windows, uint64_t* hits_fwd, uint64_t* hits_rev, size_t cap);
int gx_motif_scan_genome_group(gx_ctx* const* ctxs, int n_ctx, uint64_t* windows, uint64_t* hits_fwd, uint64_t* hits_rev, size_t cap);
int gx_motif_geometry(int* lanes, int* grid, uint32_t* positions_per_step, uint32_t* step_words, uint32_t* batch_motifs, size_t* list_cap,
                      uint64_t* flush_runs);
int gx_motif_grid(uint64_t units, uint32_t step_words, unsigned grid, unsigned* chosen);
/* From a count matrix to scores and a threshold (host only, gx_emit.cpp).
 * gx_motif_pssm: counts[b * width + j] (rows A C G T, integers below 2^31) with column sums N_j and a pseudocount pc >= 0 give
 *   scores[4 j + b] = llround(GX_MOTIF_SCALE * log2(((c + 0.25 pc) / (N_j + pc)) / 0.25)): 1/128 bit against a uniform background,
 *   halves away from zero; *smin / *smax: the least and the greatest score an L-mer can have.  GX_ERR_ORDER with a sentence in
 *   why[cap]: a width outside 1 .. 32, a count of 2^31 or more, a negative or non-finite pseudocount, a score that would be
 *   minus infinity (a zero count with pc = 0, an empty column) or leaves int16.
 * gx_motif_threshold: for p in (0, 1] let K = floor(p * 4^L) (exact: p is a double, K a 128-bit integer) and n_ge(t) the number
 *   of the 4^L L-mers whose score is >= t (a dynamic program over the columns with 128-bit counts): *threshold = the least
 *   integer t >= smin with n_ge(t) <= K; when even the greatest score has more than K L-mers, smax + 1 (the motif cannot hit) and
 *   *unreachable = 1.  *p_achieved = n_ge(t) / 4^L.  The uniform background is a stated choice (HOMER's).
 * gx_format_motif_hits: --motif-hits' table: a header, then one BED-like row per hit in the order given (sorted by region, pos,
 *   motif, strand) `chr start end ID score strand NAME peak_N offset_from_summit p_threshold`: score = "%.4f" of
 *   score / GX_MOTIF_SCALE (exact), offset_from_summit = the window's middle (2 start + L) / 2 minus the peak's summit
 *   (summit_off[k] from the peak's start, narrowPeak column 10), signed; p_threshold "%.3e" ("NA": NaN).
 * gx_format_motif_summary: --motif-summary's table: a header, then one row per motif `ID NAME width threshold p_threshold
 *   peaks_scanned peaks_with_hit windows_peaks hits_peaks windows_genome hits_genome enrichment`: peaks_scanned = the peaks at
 *   least as long as the motif, hits = both strands added, enrichment = (hits_peaks * windows_genome) / (hits_genome *
 *   windows_peaks) from two exact 128-bit products, each converted once (as gx_gc_metrics' ratios), "%.6f"; "NA" when the
 *   denominator is 0.  counts_peaks / counts_genome: [3][n_motifs] windows, hits_fwd, hits_rev.
 * gx_write_motif_hits_group / gx_write_motif_summary_group: gx_motif_scan_peaks (and, for the summary, gx_motif_scan_genome) on
 *   every context, the table of the merged peaks (see gx_write_narrowpeak_group).
 *   A context that still holds the scan of its peaks with these motifs (gx_motif_scan_peaks since the last gx_find_peaks and
 *   gx_set_motifs) is not scanned again.  gx_write_motifs_group: both tables from ONE scan of the peaks and, with summary_out,
 *   ONE genome pass (launched on every context before the first is waited for); either FILE may be NULL, not both; names may
 *   be NULL without hits_out.  counts_peaks / counts_genome (NULL: not wanted) take [3][n_motifs] windows, hits_fwd, hits_rev
 *   (the genome's zero without summary_out); *report (NULL: not wanted) the hits, the peaks with any, and the host's seconds
 *   for the peaks' scans and for the genome pass. */
typedef struct { uint64_t hits, peaks_with_hit; double peaks_seconds, genome_seconds; } gx_motif_report;
int gx_motif_pssm(const uint32_t* counts, int width, double pseudocount, int16_t* scores, int32_t* smin, int32_t* smax, char* why, size_t cap);
int gx_motif_threshold(const int16_t* scores, int width, double p, int32_t* threshold, int32_t* smin, int32_t* smax, double* p_achieved,
                       int* unreachable);
int gx_format_motif_hits(FILE* out, const char* const* names, const gx_region* peaks, const uint32_t* summit_off, size_t n_peaks,
                         const gx_motif* motifs, const char* const* ids, const char* const* motif_names, const double* p_threshold, int n_motifs,
                         const gx_motif_hit* hits, size_t n_hits);
int gx_format_motif_summary(FILE* out, const gx_region* peaks, size_t n_peaks, const gx_motif* motifs, const char* const* ids,
                            const char* const* motif_names, const double* p_threshold, int n_motifs, const gx_motif_hit* hits, size_t n_hits,
                            const uint64_t* counts_peaks, const uint64_t* counts_genome);
int gx_write_motifs_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, const gx_motif* motifs, const char* const* ids,
                          const char* const* motif_names, const double* p_threshold, int n_motifs, FILE* hits_out, FILE* summary_out,
                          uint64_t* counts_peaks, uint64_t* counts_genome, gx_motif_report* report);
int gx_write_motif_hits_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, const gx_motif* motifs, const char* const* ids,
                              const char* const* motif_names, const double* p_threshold, int n_motifs, FILE* out);
int gx_write_motif_summary_group(gx_ctx* const* ctxs, int n_ctx, const gx_motif* motifs, const char* const* ids, const char* const* motif_names,
                                 const double* p_threshold, int n_motifs, FILE* out);

/* ---- every k-mer of the called peaks counted against the whole genome (no Genrich counterpart: the counting step that HOMER,
 *      MEME-ChIP or DREME begin with, over the peak sequences cut out of the FASTA once more and a sampled background) ----
 * Needs the bases (gx_set_genome_bases); no sample, no motif.
 * k is 1 .. GX_KMER_MAX_K.  THE WINDOW at position x of a region [start, end) on chromosome c is [x, x + k).  It is COUNTED iff
 * start <= x, x + k <= min(end, len[c]) and all k acgt bits are set (the motif block's SCANNED rule with L = k).
 * THE CODE of a window is sum_j b(x + j) * 4^(k - 1 - j) with A 0, C 1, G 2, T 3: lexicographic order, the first base most
 * significant.  The device counts FORWARD codes only: counts[4^k] and windows, all exact uint64.
 * STRAND COLLAPSE happens on the host: the canonical k-mer of a code is the smaller of the code and its reverse complement
 * (gx_kmer_revcomp); its count is counts[c] + counts[rc(c)], or counts[c] alone for a palindrome.
 * Over a set of regions every region is counted on its own: overlapping regions count twice.  -E regions are NOT masked.  No
 * result depends on the launch geometry, the step, the flush bound, the table path, the split of the pushes or the number of
 * GPUs.  After every pass the host checks sum(counts) == windows; a mismatch is GX_ERR_ARR with a text, not a result.
 * Two paths: k <= GX_KMER_LDS_MAX_K counts in 4^k 32-bit LDS counters per workgroup, flushed to the 64-bit table; above it 64-bit
 * global atomics go straight into the table (gx_kmers.h).
 *
 * gx_kmer_count_regions: k_kmer_count over n regions of the caller's (any order, overlapping, empty or inverted; a chromosome
 *   outside the table, skipped or not owned counts nothing).  grid / step_words / flush_runs = 0: the library's choices; else
 *   that many workgroups (chosen or refused exactly as gx_motif_grid does), runs of 64 positions per unit (1 .. 16), and the runs
 *   a workgroup walks at most between two flushes of its LDS counters (1 .. 2^25; kept per round of four units, a round alone is
 *   always walked).  counts takes 4^k values (NULL: not wanted), windows one.  k outside 1 .. 12, no bases, a sample open or a
 *   refused geometry: GX_ERR_ORDER with a text.  For tests and measurements.
 * gx_kmer_count_peaks: after gx_find_peaks, with no sample open and the bases on (else GX_ERR_ORDER): the peaks this context
 *   called are the regions; flank < 0: the whole peaks; flank >= 0: [max(start, summit - flank), min(end, summit + flank + 1))
 *   with the summit of narrowPeak's column 10.  *regions_counted: the regions that hold at least k bases.  No peak is legal.
 *   Nothing of it is allocated or launched before the first call; its phase is "kmers".  gx_get_kmer_counts: min(cap, 4^k) of
 *   the counts.  Until gx_reset, the next sample or the next call.
 * gx_kmer_count_genome: the pass over every chromosome that takes part (the rule of gx_motif_scan_genome); min(cap, 4^k) counts.
 *   gx_kmer_count_genome_group: every context's pass is launched before the first is waited for; the counts are added.
 * gx_kmer_last: the path of the last pass (0 LDS, 1 HBM) and the flushes its workgroups made before their end.
 * gx_kmer_force_hbm: on: every k takes the HBM path (for measurements of the 7 | 8 split); it changes no result.
 * gx_kmer_geometry: the lanes of a workgroup, the most workgroups with grid = 0, the positions per step (64), the default runs
 *   per unit, the flush bound, GX_KMER_MAX_K and GX_KMER_LDS_MAX_K as the library was built.  Needs no device. */
#define GX_KMER_MAX_K 12
#define GX_KMER_LDS_MAX_K 7
int gx_kmer_count_regions(gx_ctx* ctx, const gx_region* regions, size_t n, int k, unsigned grid, uint32_t step_words, uint64_t flush_runs,
                          uint64_t* counts, uint64_t* windows);
int gx_kmer_count_peaks(gx_ctx* ctx, int k, int flank, uint64_t* windows, uint64_t* regions_counted);
int gx_get_kmer_counts(gx_ctx* ctx, uint64_t* counts, size_t cap);
int gx_kmer_count_genome(gx_ctx* ctx, int k, uint64_t* counts, size_t cap, uint64_t* windows);
int gx_kmer_count_genome_group(gx_ctx* const* ctxs, int n_ctx, int k, uint64_t* counts, size_t cap, uint64_t* windows);
int gx_kmer_last(gx_ctx* ctx, int* path, uint32_t* flushes);
int gx_kmer_force_hbm(gx_ctx* ctx, int on);
int gx_kmer_geometry(int* lanes, int* grid, uint32_t* positions_per_step, uint32_t* step_words, uint64_t* flush_runs, int* max_k, int* lds_max_k);
/* Host only (gx_emit.cpp); no context, no device.
 * gx_kmer_revcomp: the code of the reverse complement of `code` (k outside 1 .. 12 or a code of 4^k or more: 0xffffffff).
 * gx_kmer_stats: one row per canonical k-mer with count_peaks > 0.  With cp, cg its counts in the peaks and in the genome (both
 *   strands added, a palindrome once) and Wp, Wg the windows: enrichment = (cp * Wg) / (cg * Wp), two exact 128-bit products each
 *   converted to double once (NaN when cg is 0); z = (cp * Wg - cg * Wp) / sqrt(Wp * cg * (Wg - cg)), the numerator an exact
 *   signed integer, the radicand an exact integer, each converted once, then sqrt, then one division (NaN when cg is 0 or
 *   equals Wg): the binomial z-score of cp among Wp draws at rate cg / Wg.  Overlapping windows are not independent: z ranks
 *   k-mers, it is not a p-value.  Sorted by z descending with NaN last, then count_peaks descending, then code ascending.
 *   *n_rows: the rows there are; min(cap, *n_rows) are written.  A canonical count above its windows: GX_ERR_ORDER.
 * gx_format_kmers: --kmers' table: `# k=K flank=F regions=N windows_peaks=Wp windows_genome=Wg kmers=M` (F = whole for a
 *   negative flank, M the rows there are), the header `kmer revcomp count_peaks count_genome enrichment z`, then the first `top`
 *   rows (0: all); enrichment "%.6f", z "%.4f", NA for NaN.
 * gx_write_kmers_group: gx_kmer_count_peaks on every context, gx_kmer_count_genome_group, the counts added, the table. */
typedef struct { uint32_t code, revcomp; uint64_t count_peaks, count_genome; double enrichment, z; } gx_kmer_row;
typedef struct {
  uint64_t windows_peaks, windows_genome, regions_counted, kmers_counted;
  double peaks_seconds, genome_seconds;
  uint32_t top_code[3];
  double top_z[3];
  int n_top;
} gx_kmer_report;
uint32_t gx_kmer_revcomp(int k, uint32_t code);
int gx_kmer_stats(int k, const uint64_t* counts_peaks, uint64_t windows_peaks, const uint64_t* counts_genome, uint64_t windows_genome,
                  gx_kmer_row* rows, size_t cap, size_t* n_rows);
int gx_format_kmers(FILE* out, int k, int flank, uint64_t regions_counted, uint64_t windows_peaks, uint64_t windows_genome,
                    const uint64_t* counts_peaks, const uint64_t* counts_genome, int top);
int gx_write_kmers_group(gx_ctx* const* ctxs, int n_ctx, int k, int flank, int top, FILE* out, gx_kmer_report* report);

/* ---- depth distribution of each sample's pileup (no Genrich counterpart: what deepTools' plotCoverage estimates from a
 *      million sampled positions, what `samtools depth | awk` or mosdepth's distribution file take from another pass) ----
 * A sample = every gx_sample_end of the run, in call order, as for gx_get_coverage.  For one closed sample on one context:
 * a chromosome COUNTS iff it has coverage bins (not -e skipped, owned, length > 0); one the replicate's treatment header does
 * not list (save mask 0) has pileup 0 everywhere.  total = the lengths of the counting chromosomes, added; excluded = the size
 * of the union of each counting chromosome's -E regions clipped to [0, len) (they may overlap, nest, lie past the end);
 * B = total - excluded.  Every non-excluded base has a pileup v >= 0 in 1/120 units, exactly what gx_get_coverage integrates;
 * its whole depth is d = v div 120, its remainder r = v mod 120 (non-zero only with -s weights).  With GX_DEPTH_BOUND = 2048,
 * over the bases with v > 0, all exact uint64:
 *     d < GX_DEPTH_BOUND:   bases[d]    rsum[d] = sum of r    rsq[d] = sum of r^2        (class 0 holds only 0 < v < 120)
 *     d >= GX_DEPTH_BOUND:  the deep list, pairs (v, bases) with the exact v, sorted by v, one entry per distinct v
 *     min_v / max_v:        the smallest and the largest v > 0 met (0: no covered base)
 * covered = the bases with v > 0; zero = B - covered, taken by complement on the host (covered > B: GX_ERR_ARR, a lost or
 * doubled contribution, not a result).  The result is the same for every launch geometry, list capacity, push mode, tile-stage
 * path and number of contexts, whose results add (gx_depth_group: min_v / max_v combine, the deep lists merge): integers only.
 *
 * gx_set_depth_hist: on = 0: off (default).  Only while idle (after gx_create / gx_reset, before the first gx_sample_begin of a
 *   run) and after gx_set_chroms, else GX_ERR_ORDER.  Survives gx_reset; gx_saturation's child context does not inherit it.
 *   Independent of gx_set_coverage_bins and gx_set_count_in_peaks.  On, every gx_sample_end runs one more pass (k_depth_hist:
 *   gx_depth.h) over the pileup it has just closed and keeps the integers on the host until gx_reset.  When the deep list runs
 *   full the pass is run once more with a list of the counted size, while the pileup is still in place.
 * gx_depth_samples: samples closed with the switch on since the last gx_reset.
 * gx_get_depth: one sample (0 .. n_samples-1; no sample open, else GX_ERR_ORDER): *out's scalars; bases, rsum, rsq:
 *   GX_DEPTH_BOUND entries each; min(cap, *n_deep) pairs in deep_v[] / deep_bases[].  Any pointer may be NULL (the deep arrays
 *   when cap is 0); out's pointers are set to the arrays the caller passed, so that *out can go to the formatters as it is.
 * gx_depth_group: the same for sample `sample` of every context, added.  Contexts that differ in their samples: GX_ERR_ORDER.
 * gx_depth_geometry: what the edge cases depend on: the bound from which a piece is listed, the lanes of a workgroup, the most
 *   workgroups unless GX_DEPTH_GRID says otherwise, the list's first capacity.  Any pointer may be NULL.
 * gx_depth_last: the list capacity the last pass of this context ended with and how often it ran again (0 or 1). */
#define GX_DEPTH_BOUND 2048
typedef struct {
  int32_t rep, is_ctrl;
  uint64_t total, excluded, zero;
  uint64_t min_v, max_v;
  const uint64_t *bases, *rsum, *rsq;   /* [GX_DEPTH_BOUND] each */
  const uint64_t *deep_v, *deep_bases;  /* [n_deep] */
  size_t n_deep;
} gx_depth_hist;
int gx_set_depth_hist(gx_ctx* ctx, int on);
int gx_depth_samples(gx_ctx* ctx, int* n_samples);
int gx_get_depth(gx_ctx* ctx, int sample, gx_depth_hist* out, uint64_t* bases, uint64_t* rsum, uint64_t* rsq, uint64_t* deep_v,
                 uint64_t* deep_bases, size_t cap, size_t* n_deep);
int gx_depth_group(gx_ctx* const* ctxs, int n_ctx, int sample, gx_depth_hist* out, uint64_t* bases, uint64_t* rsum, uint64_t* rsq,
                   uint64_t* deep_v, uint64_t* deep_bases, size_t cap, size_t* n_deep);
int gx_depth_geometry(uint32_t* bound, int* lanes, int* grid, size_t* list_capacity);
int gx_depth_last(gx_ctx* ctx, size_t* list_capacity, int* reruns);

/* ---- peak saturation: the peaks called once more on nested subsamples of the run's own intervals (no Genrich counterpart:
 *      what a loop over `samtools view -s` and the caller answers -- would more reads have found more peaks?) ----
 * A sample = every gx_sample_end of the run in call order, as for gx_count_in_peaks; sample k's events are taken in their kept
 * order: the pushes as they came, minus the int16 rule's drops (the order gx_count_in_peaks and gx_complexity walk).  Event i
 * of sample k gets a 32-bit draw,
 *     x = seed ^ (0x9E3779B97F4A7C15 * (uint64)(k + 1));  x += i;
 *     x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31;     draw = (uint32)(x >> 32)
 * and is kept at threshold T (0 .. 2^32; more: GX_ERR_ORDER) iff draw < T: T = 2^32 keeps every event, T = 0 none, and since the
 * draw does not depend on T the subsamples of one seed are nested -- an event kept at 30 % is kept at 40 %.  The draw is keyed
 * on the position, not on the coordinates: copies of one interval are drawn independently, as reads are.  EVERY event is
 * drawn, also one on a skipped, un-saved or un-owned chromosome: i counts them all, and whoever reads the subsample applies
 * its own chromosome table, as the first run did.
 *
 * gx_subsample_draw: the draw; host only, no context.
 * gx_subsample_events: the kernels (k_sub_count, k_sub_scan, k_sub_write: gx_subsample.h) over n events in host memory (copied
 *   to the device by the call), gx_event or -- packed != 0 -- gx_event8, as sample `sample`: min(cap, kept) events into out[],
 *   always 16-byte gx_event, in their order, and *n_out = kept.  grid = 0: the library's choice, else that many workgroups (at
 *   most 65535); the output is the same bytes for every grid.  No sample open.  For tests and measurements.
 * gx_subsample_kept: the same over kept sample `sample` (0 .. n_samples-1) of a context with gx_set_count_in_peaks on.
 * gx_subsample_geometry: the lanes of a workgroup, the most workgroups with grid = 0, and the events per block (the unit the
 *   kept events are counted, scanned and written by).  Any pointer may be NULL.
 * gx_saturation: after gx_find_peaks, with gx_set_count_in_peaks on, no sample open and one context (no collectives), else
 *   GX_ERR_ORDER with a text.  For each threshold in the order given, the whole run once more on an internal child context
 *   (same device, gx_params, chromosome table, -e skips, -E coordinates, gx_set_owned mask, gx_expect_fractional and
 *   gx_set_knob values; counting, coverage, profiles off; created by the first call, gone with gx_reset / gx_destroy): per
 *   replicate the treatment's subsample with the sample's save mask, then its control WHOLE, read in place -- with
 *   GX_SAT_CONTROLS subsampled at the same threshold -- or gx_sample_no_control, then gx_pvalues; then gx_find_peaks.  out[j]:
 *   the threshold, the events of ALL the subsampled samples (n_total) and those kept (n_kept; both whole also at a point whose
 *   re-call ends early), the point's peaks, their bases,
 *   the genome length and a status.  A point whose re-call ends with GX_ERR_EXPT (the subsample left no analyzable fragment)
 *   is a result: status GX_ERR_EXPT, no peaks; every other failure fails the call, with the child's text.  The run's own
 *   peaks, counts and complexity results stay as they are; calling again gives the same.  Each kept sample takes a device
 *   buffer of its size for its subsample, from the context's pool.  A caller's device buffers must stay valid as for
 *   gx_count_in_peaks.
 * gx_get_saturation_peaks: min(cap, n_peaks) peaks of point `point` of the last gx_saturation (gx_get_peaks order).
 * gx_saturation_thresholds: the command line's points, T_j = (j << 32) / n for j = 1 .. n (the last is 2^32: the whole sample);
 *   n in 1 .. 100, else GX_ERR_ORDER; host only. */
typedef struct { uint64_t threshold, n_total, n_kept;   /* events of the subsampled samples: all, and those kept */
                 uint64_t n_peaks, peak_bp, genome_len; int32_t status; } gx_sat_point;
#define GX_SAT_CONTROLS 1u
uint32_t gx_subsample_draw(uint64_t seed, uint32_t sample, uint64_t index);
int gx_subsample_events(gx_ctx* ctx, const void* ev, size_t n, int packed, uint64_t seed, uint32_t sample, uint64_t threshold,
                        unsigned grid, gx_event* out, size_t cap, size_t* n_out);
int gx_subsample_kept(gx_ctx* ctx, int sample, uint64_t seed, uint64_t threshold, gx_event* out, size_t cap, size_t* n_out);
int gx_subsample_geometry(int* lanes, int* grid, uint32_t* block_events);
int gx_saturation(gx_ctx* ctx, const uint64_t* threshold, int n_points, uint64_t seed, unsigned flags, gx_sat_point* out);
int gx_get_saturation_peaks(gx_ctx* ctx, int point, gx_peak* out, size_t cap);
int gx_saturation_thresholds(int n_points, uint64_t* threshold);

/* ---- peak reproducibility over (pseudo-)replicates: the peaks called once more on every replicate alone, on two random
 *      halves of every replicate and on the two pools of halves (no Genrich counterpart: what ENCODE's 3R + 2 further runs of
 *      the caller on `samtools view -s` halves answer -- are these peaks one replicate's work?) ----
 * The halves are the subsample's (above): event i of kept sample k is in half A iff its draw is below T, else in half B, so
 * half A at T is exactly gx_subsample_kept(k, seed, T) and B is its complement, both in kept order.
 *
 * gx_subsample_split_events: the kernels (k_sub_count, k_sub_scan, k_sub_split: gx_subsample.h) over n events in host memory,
 *   as gx_subsample_events takes them (the same argument rules and refusals): min(cap, n) events into out[], half A in
 *   [0, *n_a), half B behind it, always 16-byte gx_event; the same bytes for every grid.  For tests and measurements.
 * gx_subsample_split_kept: the same over kept sample `sample` of a context with gx_set_count_in_peaks on.
 * gx_reproducibility: after gx_find_peaks, with gx_set_count_in_peaks on, no sample open and one context, else GX_ERR_ORDER
 *   with a text; flags must be 0.  Each treatment is split once at T = 2^31 (its kept index is the draw's sample); controls
 *   are never split.  Then 3R + 2 calls on gx_saturation's child context, in this order, R = the replicates:
 *     GX_REPRO_ALONE r, r = 0 .. R-1: replicate r whole with its save mask and its control (or none), as a one-replicate run;
 *     GX_REPRO_SELF r h, h = 0, 1:    half h of replicate r with the same control, as a one-replicate run;
 *     GX_REPRO_POOLED h, h = 0, 1:    half h of EVERY replicate, each with its own control and save mask, combined as the run
 *                                     combines its replicates: the run itself on half the treatment intervals.
 *   With R = 1 all five are made: ALONE 0 is the run itself and POOLED h equals SELF 0 h.  out[i], i < min(cap, 3R + 2), and
 *   *n_calls = 3R + 2: the call's kind, replicate (-1: pooled) and half (-1: alone), the treatment events pushed, its peaks and
 *   their bases, and a status: GX_ERR_EXPT where the call left no analyzable fragment -- a result, with an empty list; every
 *   other failure fails the whole call, with "reproducibility: " before the child's text.  The run's own peaks, counts and
 *   complexity results stay as they are; calling again gives the same; gx_reset drops the result.
 * gx_get_reproducibility_peaks: min(cap, n_peaks) peaks of call `call` of the last gx_reproducibility (gx_get_peaks order). */
#define GX_REPRO_ALONE 0
#define GX_REPRO_SELF 1
#define GX_REPRO_POOLED 2
typedef struct { int32_t kind, rep, half, status; uint64_t n_events, n_peaks, peak_bp; } gx_repro_call;
int gx_subsample_split_events(gx_ctx* ctx, const void* ev, size_t n, int packed, uint64_t seed, uint32_t sample, uint64_t threshold,
                              unsigned grid, gx_event* out, size_t cap, size_t* n_a);
int gx_subsample_split_kept(gx_ctx* ctx, int sample, uint64_t seed, uint64_t threshold, gx_event* out, size_t cap, size_t* n_a);
int gx_reproducibility(gx_ctx* ctx, uint64_t seed, unsigned flags, gx_repro_call* out, size_t cap, size_t* n_calls);
int gx_get_reproducibility_peaks(gx_ctx* ctx, int call, gx_peak* out, size_t cap);

/* ---- signal profiles around anchor sites per sample (no Genrich counterpart: the integral of gx_get_coverage, taken over
 *      strand-oriented windows around given positions instead of fixed genome-wide bins; the aggregate around transcription
 *      start sites is the TSS-enrichment curve) ----
 * An anchor is (chrom, pos, strand), strand +1 or -1.  With the flank F and the bin size B (B >= 1, F % B == 0) an anchor has
 * nb = 2 F / B bins (nb <= 1024).  Bin j (0 <= j < nb) covers these bases x of the anchor's chromosome:
 *     strand +:  pos - F + j B       <= x <  pos - F + (j + 1) B
 *     strand -:  pos + F - (j + 1) B <  x <= pos + F - j B            (the mirror image)
 * so that on both strands the anchor base is the first base, in reading direction, of bin nb / 2.
 * cell120[a][j] is the sum over the bases of bin j of anchor a of the sample's pileup there, in 1/120 units, an exact int64.
 * The pileup is the one gx_get_coverage integrates: a treatment's `experimental` pileup; a control's own raw pileup, before
 * factor and lambda; 0 inside -E regions.  Bases x < 0 or x >= len count 0.  A row is all zeros when the anchor's chromosome is
 * skipped (-e), empty or not owned by this context (gx_set_owned), when the replicate's save mask leaves it out, or when its
 * index lies behind the table (chrom >= nChrom); an anchor with pos >= len on a known chromosome is legal and covers whatever
 * part of its window is inside.  agg120[j] is the sum of cell120[a][j] over all anchors.  Everything is an integer: a result
 * does not depend on the grid, on the order of the adds or on the number of contexts, and a host adds the contexts' rows and
 * aggregates as it does for region counts.  A sample = every gx_sample_end of the run, in call order, as for gx_get_coverage.
 *
 * gx_set_profile: n == 0 = off (default).  Only while idle (after gx_create / gx_reset, before the first gx_sample_begin) and
 *   after gx_set_chroms, else GX_ERR_ORDER; also GX_ERR_ORDER: bin_size == 0, flank == 0 or flank > 2^20,
 *   flank % bin_size != 0, nb > 1024, a strand other than +1 / -1, with keep_matrix more than 2^26 cells (n * nb).  The anchors
 *   are copied.  Survives gx_reset, like gx_set_coverage_bins.  On, every gx_sample_end runs k_profile and k_profile_sum
 *   (gx_profile.h) over the pileup it has just closed and keeps nb int64 -- with keep_matrix n * nb more -- in device memory
 *   until gx_reset (a failed allocation: GX_ERR_MEM); off, a run launches and allocates nothing for it.
 * gx_profile_samples: samples closed with the profile on since the last gx_reset.
 * gx_profile_layout: what gx_set_profile was given (any pointer may be NULL); all zero while off.
 * gx_get_profile: one sample's (0 .. n_samples-1) replicate, whether it is a control, its aggregate (n_bins values, or NULL) and
 *   n_rows rows of its matrix from first_anchor on, in the caller's anchor order (n_rows * n_bins values, or NULL).  Rows when no
 *   matrix was kept, rows beyond the anchors, a bad index or a sample still open: GX_ERR_ORDER.  It needs no gx_pvalues and no
 *   gx_find_peaks. */
typedef struct {
  uint32_t chrom, pos;
  int32_t strand;
} gx_anchor;
int gx_set_profile(gx_ctx* ctx, const gx_anchor* anchors, size_t n, uint32_t flank, uint32_t bin_size, int keep_matrix);
int gx_profile_samples(gx_ctx* ctx, int* n_samples);
int gx_profile_layout(gx_ctx* ctx, size_t* n_anchors, uint32_t* n_bins, uint32_t* flank, uint32_t* bin_size, int* has_matrix);
int gx_get_profile(gx_ctx* ctx, int sample, int* rep, int* is_ctrl, int64_t* agg120, int64_t* cell120, size_t first_anchor,
                   size_t n_rows);

/* ---- host-side text emitters of the drop-in surface (gx_emit.cpp); byte format of the
 *      reference's printf calls.  names[i] = chromosome names in table order. ---- */
#include <stdio.h>
/* -o  ENCODE narrowPeak: printPeak, Genrich.c:885-909 */
int gx_write_narrowpeak(gx_ctx* ctx, const char* const* names, FILE* out);
/* -k  pileup log of replicate rep: printPileHeader 1680-1691, printPile 1697-1715 */
int gx_write_pile(gx_ctx* ctx, int rep, const char* const* names, int n_chrom, const char* expt_name,
                  const char* ctrl_name, FILE* out);
/* -f  bedgraph-ish log: printLogHeader 674-717, printInterval 770-803, printIntervalN 724-763;
 *     peaks_opt = 0 is -X (logIntervals 837-878) */
int gx_write_log(gx_ctx* ctx, int n_rep, const char* const* names, int n_chrom, int qval_opt, int peaks_opt,
                 float thr, FILE* out);
/* The same for a run whose chromosomes are sharded over several contexts (one per GPU); owner[c] = index into ctxs of
 * the context that computed chromosome c.
 * THE MERGED PEAKS: every group writer with a row (or a group of rows) per called peak -- gx_write_narrowpeak_group,
 * gx_write_counts_group, gx_write_peak_signal_group, gx_write_summits_group, gx_write_gc_peaks_group, gx_write_motifs_group --
 * numbers the peaks alike: the contexts' lists (gx_get_peaks) concatenated in the order of ctxs, then, for n_ctx > 1,
 * stable-sorted by (chrom, start) -- chromosome-table order, then position, the order in which the reference meets them
 * (Genrich.c:986, 925); one context's list is taken as it is.  Merged peak i is peak_i in every file of a run. */
int gx_write_narrowpeak_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, FILE* out);
int gx_write_pile_group(gx_ctx* const* ctxs, const int* owner, int rep, const char* const* names, int n_chrom,
                        const char* expt_name, const char* ctrl_name, FILE* out);
int gx_write_log_group(gx_ctx* const* ctxs, const int* owner, int n_rep, const char* const* names, int n_chrom,
                       int qval_opt, int peaks_opt, float thr, FILE* out);
int gx_write_narrowpeak_path(gx_ctx* ctx, const char* const* names, const char* path);
/* --counts (no Genrich counterpart; after gx_count_in_peaks on every context): a header "chr\tstart\tend\tname" and one
 * column per sample (sample_names[i], n_samples of them), then one row per narrowPeak line (the merged peaks); a value n (1/120 units) is printed as n / 120 with %lld when n % 120 == 0, else with
 * %.2f. */
int gx_write_counts_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, int n_samples,
                          const char* const* sample_names, FILE* out);
int gx_write_counts(gx_ctx* ctx, const char* const* names, int n_samples, const char* const* sample_names, FILE* out);
int gx_write_counts_path(gx_ctx* ctx, const char* const* names, int n_samples, const char* const* sample_names,
                         const char* path);
/* --region-counts (after gx_count_in_regions with the same regions on every context): the header of --counts, then exactly one
 * row per region in the caller's order -- names[chrom], start and end as given (not clamped), region_names[k] or, where that (or
 * region_names) is NULL, region_N with N = k -- with the contexts' counts added, printed as --counts prints them.  names must
 * reach every chrom the regions use: a caller gives unknown chromosomes indices behind the table and their names there. */
int gx_write_region_counts_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, const gx_region* regions,
                                 const char* const* region_names, size_t n, int n_samples, const char* const* sample_names,
                                 FILE* out);
int gx_write_region_counts(gx_ctx* ctx, const char* const* names, const gx_region* regions, const char* const* region_names,
                           size_t n, int n_samples, const char* const* sample_names, FILE* out);
int gx_write_region_counts_path(gx_ctx* ctx, const char* const* names, const gx_region* regions, const char* const* region_names,
                                size_t n, int n_samples, const char* const* sample_names, const char* path);
/* --peak-signal (no Genrich counterpart).  gx_format_peak_signal: host only, no context.  A header "chr\tstart\tend\tname" and
 * per sample the five columns <label>.max <label>.summit <label>.area <label>.covered <label>.at_summit, <label> = t<rep> or
 * c<rep>; then one row per peak in the order given: names[chrom], start, end, peak_N with N = k, and the samples' figures --
 * those in 1/120 units printed as --counts prints a count (n / 120 with %lld when n % 120 == 0, else %.2f), summit and covered
 * as they are.  n_peaks == 0 and n_samples == 0 are legal.  gx_write_peak_signal_group: runs gx_peak_signal on every context
 * and formats the merged peaks; contexts that differ in their samples:
 * GX_ERR_ORDER.  gx_write_peak_signal: one context. */
int gx_format_peak_signal(FILE* out, const char* const* names, const gx_region* peaks, size_t n_peaks, int n_samples,
                          const int* rep, const int* is_ctrl, const int64_t* const* area120, const int64_t* const* max120,
                          const uint32_t* const* summit, const uint32_t* const* covered, const int64_t* const* at_summit120);
int gx_write_peak_signal_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, FILE* out);
int gx_write_peak_signal(gx_ctx* ctx, const char* const* names, FILE* out);
/* --summits (no Genrich counterpart).  gx_format_summits: host only, no context.  The header
 * "chr\tstart\tend\tname\theight\tstrand\tplateau_start\tplateau_end\tprominence\tpeak_start\tpeak_end", then one row per summit
 * (ascending in (peak, pos), else GX_ERR_ORDER): names[chrom], summit, summit + 1, peak_N.j with N the peak's index and j = 1,
 * 2, ... from left to right within it, the height, ".", the plateau [start, end), the prominence, the peak's start and end --
 * narrowPeak coordinates; height and prominence printed as --counts prints a count.  n == 0 is legal.
 * gx_write_summits_group: runs gx_peak_summits on every context and formats the merged peaks.  gx_write_summits: one context. */
int gx_format_summits(FILE* out, const char* const* names, const gx_region* peaks, size_t n_peaks, const gx_summit* summits,
                      size_t n);
int gx_write_summits_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, int prominence_pct, int height_pct, FILE* out);
int gx_write_summits(gx_ctx* ctx, const char* const* names, int prominence_pct, int height_pct, FILE* out);
/* --coverage (no Genrich counterpart; printPile 1697 is what -k prints instead): bedGraph without a header line.
 * gx_format_coverage: host only, no context.  One chromosome's bins (n_bins = ceil(len / bin_size) sums in 1/120 units) as lines
 * "chrom\tstart\tend\tvalue\n" that tile [0, len) with no gap and no overlap, zero runs included.  Adjacent bins are merged
 * into one line iff their means are exactly equal (sum_a * bases_b == sum_b * bases_a, compared in 128-bit integers).  The
 * value of a line over `bases` bases with the sum `sum`: when scale == 1.0 and sum % (120 * bases) == 0 the integer
 * sum / (120 * bases) with %lld, otherwise %.4f of ((double)sum / (120.0 * (double)bases)) * scale, evaluated in that order.
 * n_bins != ceil(len / bin_size), bin_size == 0 or a missing pointer: GX_ERR_ORDER, nothing written.
 * gx_write_coverage: one sample (gx_get_coverage's index) over the chromosomes in table order, those without bins left out;
 * _group: owner[c] = index into ctxs of the context that computed chromosome c (NULL: ctxs[0]), as gx_write_pile_group. */
int gx_format_coverage(FILE* out, const char* chrom_name, uint32_t len, uint32_t bin_size, const int64_t* sum120,
                       size_t n_bins, double scale);
int gx_write_coverage_group(gx_ctx* const* ctxs, const int* owner, int sample, const char* const* names, int n_chrom,
                            double scale, FILE* out);
int gx_write_coverage(gx_ctx* ctx, int sample, const char* const* names, int n_chrom, double scale, FILE* out);
int gx_write_coverage_path(gx_ctx* ctx, int sample, const char* const* names, int n_chrom, double scale, const char* path);
/* --profile (no Genrich counterpart).  gx_format_profile and gx_format_profile_rows: host only, no context.
 * gx_format_profile: the aggregate table -- "offset" and one column per sample, then n_bins rows: the bin's first offset
 * -flank + j bin_size, then per sample %.6f of (double)agg120[s][j] / (120.0 * bin_size * n_anchors_counted), evaluated in that
 * order (0.000000 when n_anchors_counted is 0).  n_anchors_counted is the caller's: the anchors on chromosomes the run computes.
 * gx_format_profile_rows: n_rows matrix rows, anchors first .. first + n_rows - 1 (regions, row_names and anchors are indexed by
 * anchor, cell120 by row): "chrom\tstart\tend\tname\tstrand" of the anchor's BED line -- names[regions[a].chrom], the name
 * "anchor_<a>" where row_names or row_names[a] is NULL, the strand "+" or "-" -- then n_bins values: the integer
 * cell / (120 bin_size) with %lld when it is one, else %.4f of (double)cell / (120.0 * bin_size).
 * A missing pointer, n_bins == 0 or bin_size == 0: GX_ERR_ORDER, nothing written.
 * _group (gx_api.hip: they read contexts): the contexts' aggregates / rows added, as gx_write_region_counts_group adds counts;
 * the layout is ctxs[0]'s. */
int gx_format_profile(FILE* out, int n_samples, const char* const* sample_names, const int64_t* const* agg120,
                      size_t n_anchors_counted, uint32_t n_bins, uint32_t flank, uint32_t bin_size);
int gx_format_profile_rows(FILE* out, const char* const* names, const gx_region* regions, const char* const* row_names,
                           const gx_anchor* anchors, size_t first, size_t n_rows, uint32_t n_bins, uint32_t bin_size,
                           const int64_t* cell120);
int gx_write_profile_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, const char* const* sample_names,
                           size_t n_anchors_counted, FILE* out);
int gx_write_profile_rows_group(gx_ctx* const* ctxs, int n_ctx, int sample, const char* const* names, const gx_region* regions,
                                const char* const* row_names, const gx_anchor* anchors, FILE* out);
/* --correlation (no Genrich counterpart).  gx_format_correlation: host only, no context.  The Pearson matrix of the sums of
 * gx_coverage_gram (gram[n_samples * n_samples], row-major): with N = n, or n - n_zero when skip_zeros,
 *     r_ij = (N g_ij - s_i s_j) / sqrt((N g_ii - s_i^2) (N g_jj - s_j^2)).
 * The three differences are exact 256-bit integers (N g < 2^156, s_i s_j < 2^162: two numbers of 150 bits cancel there); only
 * they are converted to double.  A TSV: the header line is a tab and the sample names, then per sample its name and S values
 * %.6f; the diagonal is 1.000000; a pair with a sample of zero variance, and every pair when N < 2, is "nan".
 * A missing pointer or n_samples < 1: GX_ERR_ORDER, nothing written.
 * gx_correlation_matrix: the same r as doubles, r[n_samples * n_samples] row-major, NaN where the text says "nan" (host only).
 * gx_coverage_gram_group (gx_api.hip: it reads contexts): gx_coverage_gram of every context, added with carries; sum[n_samples]
 * and gram[n_samples * n_samples] are required.  gx_write_correlation_group: that, then gx_format_correlation. */
int gx_correlation_matrix(int n_samples, uint64_t n, uint64_t n_zero, const gx_u128* sum, const gx_u128* gram, int skip_zeros,
                          double* r);
int gx_coverage_gram_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, uint64_t* n_bins, uint64_t* n_zero, gx_u128* sum,
                           gx_u128* gram);
int gx_format_correlation(FILE* out, int n_samples, const char* const* sample_names, uint64_t n, uint64_t n_zero,
                          const gx_u128* sum, const gx_u128* gram, int skip_zeros);
int gx_write_correlation_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, const char* const* sample_names, int skip_zeros,
                               FILE* out);
/* --spearman (no Genrich counterpart; defined with gx_coverage_spearman_group above): --correlation's text, of the rank rows */
int gx_write_spearman_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, const char* const* sample_names, int skip_zeros, FILE* out);
/* --fingerprint (no Genrich counterpart).  The first three: host only, no context; count and sum are [n_samples][GX_FP_NC] as
 * gx_coverage_fingerprint gives them, ctrl_of[s] is the sample index of s's control or -1 (ctrl_of == NULL: all -1).
 * gx_fingerprint_metrics: the figures defined above, NaN where they are not.
 * gx_format_fingerprint: a TSV with the header "sample lo120 hi120 bins sum120 cum_bins cum_signal" and one row per sample and
 *   non-empty class in ascending order: the class's lo and hi, its count and sum as integers, C_k / n and T_k / T as %.6f
 *   ("nan" with T == 0).
 * gx_format_fingerprint_metrics: header "sample bins zero_bins sum120 zero_fraction auc gini elbow_bins elbow_gap jsd_control",
 *   one row per sample: n, count[0] and T as integers, the figures as %.6f or "nan".
 * A missing pointer, n_samples < 1 or a ctrl_of entry that is not a sample other than s: GX_ERR_ORDER, nothing written.
 * gx_coverage_fingerprint_group (gx_api.hip: it reads contexts): gx_coverage_fingerprint of every context, added; count and
 * sum are required.  gx_write_fingerprint_group: that, then the curve table to `curve` and, unless NULL, the figures to `metrics`. */
int gx_fingerprint_metrics(int n_samples, const uint64_t* count, const uint64_t* sum, const int* ctrl_of, gx_fp_metrics* out);
int gx_format_fingerprint(FILE* out, int n_samples, const char* const* sample_names, const uint64_t* count, const uint64_t* sum);
int gx_format_fingerprint_metrics(FILE* out, int n_samples, const char* const* sample_names, const uint64_t* count,
                                  const uint64_t* sum, const int* ctrl_of);
int gx_coverage_fingerprint_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, uint64_t* n_bins, uint64_t* count, uint64_t* sum);
int gx_write_fingerprint_group(gx_ctx* const* ctxs, int n_ctx, int n_samples, const char* const* sample_names, const int* ctrl_of,
                               FILE* curve, FILE* metrics);
/* --complexity (no Genrich counterpart).  The first three: host only, no context.  A sample's histogram is n_pairs pairs
 * (mult[i], keys[i]), mult strictly ascending and >= 1, keys >= 1, with sum keys = D and sum mult keys = N (else GX_ERR_ORDER).
 * gx_complexity_metrics, with h1 = h[1] and h2 = h[2]:
 *     nrf = D / N        pbc1 = h1 / D        pbc2 = h1 / h2        dup_fraction = (N - D) / N
 *   each ONE division of two integers (the correctly rounded double while both are below 2^53), NaN where the divisor is 0;
 *     library_size = the X with D / X = 1 - exp(-N / X) (Lander-Waterman: what Picard prints), by bisection with expm1 in long
 *   double, rounded to an integer; NaN when D == N or N == 0;
 *     curve[k - 1], k = 1 .. GX_CPX_CURVE = 20: with n = floor((k N + 10) / 20), i.e. round(0.05 k N) with halves up, the expected
 *   number of distinct keys among n of the N observations drawn without replacement,
 *     E_n = sum_m h[m] (1 - prod_{i=0}^{m-1} (N - n - i) / (N - i)),
 *   the product taken factor by factor in long double and stopped once it is 0 or below 2^-80 (then 1 - p is 1); E_N = D exactly,
 *   and every point is 0 when N == 0.
 * gx_format_complexity: a TSV, header "sample N D h1 h2 NRF PBC1 PBC2 dup_fraction library_size c005 c010 ... c100", one row
 *   per sample labelled t<rep> / c<rep>: the integers, the four ratios as %.6f, the library size as an integer, the curve's
 *   points as %.3f; a figure that is not defined prints as NA.
 * gx_format_complexity_hist: header "sample multiplicity keys", one row per sample and pair.
 * A missing pointer or n_samples < 1: GX_ERR_ORDER, nothing written.
 * gx_write_complexity_group (gx_api.hip: it reads contexts): gx_complexity on every context, gx_complexity_group per sample,
 *   then the figures to `metrics` and, unless NULL, the histogram to `hist`. */
#define GX_CPX_CURVE 20
typedef struct {
  uint64_t h1, h2;
  double nrf, pbc1, pbc2, dup_fraction, library_size;
  double curve[GX_CPX_CURVE];
} gx_cpx_metrics;
int gx_complexity_metrics(uint64_t n_obs, uint64_t n_distinct, const uint64_t* mult, const uint64_t* keys, size_t n_pairs,
                          gx_cpx_metrics* out);
int gx_format_complexity(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* n_obs,
                         const uint64_t* n_distinct, const uint64_t* const* mult, const uint64_t* const* keys, const size_t* n_pairs);
int gx_format_complexity_hist(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* const* mult,
                              const uint64_t* const* keys, const size_t* n_pairs);
int gx_write_complexity_group(gx_ctx* const* ctxs, int n_ctx, FILE* metrics, FILE* hist);
/* --lengths / --lengths-metrics / --chrom-stats (no Genrich counterpart).  The first four: host only, no context.  A sample's
 * lengths are n_classes entries (length[i], n[i], w120[i]): length strictly ascending and below 2^32, n >= 1, n <= w120 <= 120 n
 * (else GX_ERR_ORDER).  cuts: n_cuts <= GX_LEN_MAX_CUTS strictly ascending positive lengths.
 * gx_lengths_metrics, every figure over WEIGHT (W = sum w120): n = sum n; mean = sum w L / W and sd = sqrt(W sum w L^2 -
 *   (sum w L)^2) / W (population) from exact 128- / 256-bit sums, doubles only at the end, NaN for an empty sample; min, max;
 *   mode = the smallest L of the greatest weight; p5, q25, median, q75, p95 = the smallest L whose cumulative weight times 100
 *   is >= q W, in integers; share[k], k = 0 .. n_cuts: the share of W with cuts[k - 1] <= L < cuts[k] (150,300,500: the
 *   nucleosome-free / mono- / di-nucleosome / longer reading of an ATAC library).  Inverted intervals take no part.
 * gx_format_lengths: a comment line that says what an interval is (cut_sites != 0: the cut-site windows of -j), then a TSV, header
 *   "sample length intervals weight cum_weight_share", one row per sample (t<rep> / c<rep>) and length; weight as --counts prints
 *   a 1/120 value (an integer, else %.2f), the share as %.6f of the sample's W; then one row "inverted" per sample that has any
 *   (share NA).
 * gx_format_lengths_metrics: header "sample intervals weight mean sd min p5 q25 median q75 p95 max mode lt<A> ge<A>_lt<B> ...
 *   ge<Z>", one row per sample; mean and sd %.6f (NA when empty), shares %.6f.
 * gx_format_chrom_stats: a comment line, then header "chrom length" and per sample "<s>.intervals <s>.weight <s>.share
 *   <s>.mean_depth"; one row per chromosome in table order; share = cw120 over the sample's whole weight, mean_depth =
 *   cbases120 / (120 length), both %.6f (0 when the divisor is 0).  A chromosome skipped with -e: zeros.
 * gx_write_interval_stats_group (gx_api.hip: it reads contexts): gx_interval_stats on every context, the group sums per
 *   sample, then whichever of the three files is not NULL (at least one). */
#define GX_LEN_MAX_CUTS 8
typedef struct {
  uint64_t n, w120;
  uint64_t min, max, mode, p5, q25, median, q75, p95;
  double mean, sd;
  int n_shares;
  double share[GX_LEN_MAX_CUTS + 1];
} gx_len_metrics;
int gx_lengths_metrics(const uint64_t* length, const uint64_t* n, const uint64_t* w120, size_t n_classes, const uint64_t* cuts, int n_cuts,
                       gx_len_metrics* out);
int gx_format_lengths(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* const* length, const uint64_t* const* n,
                      const uint64_t* const* w120, const size_t* n_classes, const uint64_t* n_inverted, const uint64_t* w120_inverted,
                      int cut_sites);
int gx_format_lengths_metrics(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* const* length,
                              const uint64_t* const* n, const uint64_t* const* w120, const size_t* n_classes, const uint64_t* cuts, int n_cuts);
int gx_format_chrom_stats(FILE* out, const char* const* names, const uint32_t* lens, int n_chrom, int n_samples, const int* rep,
                          const int* is_ctrl, const uint64_t* const* cn, const uint64_t* const* cw120, const uint64_t* const* cbases120);
int gx_write_interval_stats_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, int n_chrom, int cut_sites, const uint64_t* cuts,
                                  int n_cuts, FILE* lengths, FILE* metrics, FILE* chroms);
/* --xcor / --xcor-metrics (no Genrich counterpart).  All but the last: host only, no context.  A sample's counts must be
 * consistent (n_plus, n_minus <= n_pos, every n11 <= min(n_plus, n_minus), -GX_XCOR_MAX_SHIFT <= lo <= hi <= GX_XCOR_MAX_SHIFT),
 * else GX_ERR_ORDER, nothing written.
 * gx_xcor_metrics, read_len = R > 0 or 0 for none; the phantom shift is ph = R - 1:
 *   frag_shift = the smallest d with the greatest r(d) among max(1, lo) <= d <= hi, without those with |d - ph| <= 10 when R is
 *     given; fragment_length = frag_shift + 1; r_frag = r(frag_shift).  has_frag = 0 (and NaN) when no such d exists or r is NaN.
 *   min_shift, r_min = the smallest d with the least r(d) over the whole range.
 *   nsc = r_frag / r_min, NaN unless r_min > 0.  rsc = (r_frag - r_min) / (r(ph) - r_min), NaN without R, with ph outside
 *     [lo, hi] or when the denominator is <= 0.  has_phantom: R given and ph inside the range (r_phantom = r(ph)).  No smoothing.
 * gx_xcor_r: r(d) alone, hi - lo + 1 doubles.
 * gx_format_xcor: header "sample shift n11 r", then per sample (t<rep> / c<rep>) a line "# <sample> n_pos=.. n_plus=.. n_minus=..
 *   rejected=.." and one row per shift; r as %.6f, NA where undefined.
 * gx_format_xcor_metrics: header "sample n_pos n_plus n_minus fragment_length r_frag min_shift r_min phantom_shift r_phantom NSC
 *   RSC", one row per sample; doubles %.6f; NA where undefined.
 * gx_write_xcor_group (gx_api.hip: it reads contexts): the group sums per sample, then whichever of the two files is not NULL. */
typedef struct {
  int has_frag, frag_shift, fragment_length;
  int min_shift;
  int has_phantom, phantom_shift;
  int pad_;
  double r_frag, r_min, r_phantom, nsc, rsc;
} gx_xcor_metrics_t;
int gx_xcor_metrics(uint64_t n_pos, uint64_t n_plus, uint64_t n_minus, int lo, int hi, const uint64_t* n11, int read_len, gx_xcor_metrics_t* out);
int gx_xcor_r(uint64_t n_pos, uint64_t n_plus, uint64_t n_minus, int lo, int hi, const uint64_t* n11, double* r);   /* r[hi - lo + 1] */
int gx_format_xcor(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* n_pos, const uint64_t* n_plus,
                   const uint64_t* n_minus, const uint64_t* rejected, int lo, int hi, const uint64_t* const* n11);
int gx_format_xcor_metrics(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* n_pos, const uint64_t* n_plus,
                           const uint64_t* n_minus, int lo, int hi, const uint64_t* const* n11, int read_len);
int gx_write_xcor_group(gx_ctx* const* ctxs, int n_ctx, int read_len, FILE* curve, FILE* metrics);
/* --depth / --depth-metrics (no Genrich counterpart).  The first three: host only, no context.  A histogram that contradicts
 * itself (a missing array, excluded > total, covered + zero != B, rsum[d] > 119 bases[d], a deep list that is not strictly
 * ascending from 120 GX_DEPTH_BOUND, covered bases without min_v <= max_v): GX_ERR_ORDER, nothing written.
 * gx_depth_metrics: from the integers, every sum an exact big integer before anything becomes a double:
 *     sum v   = sum_d (120 d bases[d] + rsum[d]) + sum_deep v bases
 *     sum v^2 = sum_d (14400 d^2 bases[d] + 240 d rsum[d] + rsq[d]) + sum_deep v^2 bases
 *   bases = B, covered, covered_fraction = covered / B, mean = sum v / (120 B), sd = sqrt(B sum v^2 - (sum v)^2) / (120 B)
 *   (population; mean and sd NaN when B = 0, every fraction 0 then); min_v / max_v: the exact smallest and largest pileup over
 *   the B bases in 1/120 units (min_v 0 when a base is at 0); q25 .. p99: the smallest whole depth d with
 *   100 #(bases of depth <= d) >= q B, in integers; ge[k]: the fraction of B at whole depth >= 1, 2, 5, 10, 20, 50, 100.
 * gx_format_depth: a TSV, header "#sample depth bases bases_at_least fraction_at_least", per sample (labelled t<rep> / c<rep>)
 *   one row per non-empty whole depth, ascending; the depth-0 row is always there and includes the bases at pileup 0; deep
 *   entries are grouped by v div 120; fraction_at_least is %.6f of B, 0.000000 when B = 0.
 * gx_format_depth_metrics: header "sample bases excluded covered covered_fraction mean sd min q25 median q75 p95 p99 max ge1 ge2
 *   ge5 ge10 ge20 ge50 ge100", one row per sample; fractions, mean and sd as %.6f (NA when not defined), min and max as --coverage
 *   prints a value (an integer when v divides by 120, else %.4f).
 * gx_write_depth_group (gx_api.hip: it reads contexts): gx_depth_group per sample, then the distribution to `depth` and the
 *   figures to `metrics`; either may be NULL, not both. */
#define GX_DEPTH_NGE 7
typedef struct {
  uint64_t bases, excluded, covered;
  uint64_t min_v, max_v;
  uint64_t q25, median, q75, p95, p99;
  double covered_fraction, mean, sd;
  double ge[GX_DEPTH_NGE];
} gx_depth_metrics_t;
int gx_depth_metrics(const gx_depth_hist* hist, gx_depth_metrics_t* out);
int gx_format_depth(FILE* out, int n_samples, const gx_depth_hist* hist);
int gx_format_depth_metrics(FILE* out, int n_samples, const gx_depth_hist* hist);
int gx_write_depth_group(gx_ctx* const* ctxs, int n_ctx, FILE* depth, FILE* metrics);
/* --saturation (no Genrich counterpart).  The first two: host only, no context.
 * gx_saturation_overlap: two peak lists in gx_get_peaks order (by chromosome, then start; no overlaps inside a list), in one
 *   merge walk, with gx_count_in_peaks' predicate (s < pe && ps < e on one chromosome): *full_recovered = the peaks of `full`
 *   touched by at least one peak of `sub`, *sub_in_full = the peaks of `sub` touched by at least one of `full`, *shared_bp =
 *   the bases both lists cover.  Any out pointer may be NULL.
 * gx_format_saturation: a comment line "# run: <n_full> peaks, <full_bp> bp", then a TSV, header "fraction threshold kept peaks
 *   peak_bp recovered recovered_share in_run shared_bp status", one row per point: the threshold over 2^32 as %.6f, the threshold, the intervals kept, the point's peaks and
 *   their bases, the run's peaks it recovers and the same over n_full as %.6f (NA when the run has none), the point's peaks
 *   that touch one of the run's, the shared bases, and "ok" or, for GX_ERR_EXPT, "no_fragments" (another status: its number).
 *   A missing pointer or n_points < 1: GX_ERR_ORDER, nothing written.
 * gx_write_saturation (gx_api.hip: it reads a context): the last gx_saturation against the run's own peaks. */
int gx_saturation_overlap(const gx_peak* full, size_t n_full, const gx_peak* sub, size_t n_sub, uint64_t* full_recovered,
                          uint64_t* sub_in_full, uint64_t* shared_bp);
int gx_format_saturation(FILE* out, int n_points, const gx_sat_point* points, const uint64_t* full_recovered,
                         const uint64_t* sub_in_full, const uint64_t* shared_bp, uint64_t n_full, uint64_t full_bp);
int gx_write_saturation(gx_ctx* ctx, FILE* out);
/* --reproducibility (no Genrich counterpart).  All but the last: host only, no context.
 * gx_peaks_supported: two peak lists in gx_get_peaks order (by chromosome, then start; no overlaps inside a list), in one
 *   merge walk: hit[i] = 1 iff some b[j] on a[i]'s chromosome overlaps it by ov >= 1 bases with 100 * ov >= pct *
 *   min(len a[i], len b[j]), in exact 64-bit integers.  pct: 0 .. 100 (else GX_ERR_ORDER); 0 = "touches", 50 = ENCODE's "half
 *   of either peak", 100 = the shorter lies inside the longer.
 * gx_reproducibility_figures: from the run's peaks, gx_reproducibility's 3 R + 2 calls (in its order, else GX_ERR_ORDER) and
 *   their peak lists.  nt_pair[R (R-1) / 2], pairs i < j in row order: the run's peaks supported by both ALONE i and ALONE j;
 *   Nt the greatest, with its pair (a tie: the first).  n_self[R]: ALONE r's peaks supported by both SELF r 0 and SELF r 1.
 *   Np: the run's peaks supported by both pooled calls.  rescue = max(Np, Nt) / min(Np, Nt), self_consistency = max n_self /
 *   min n_self; a ratio has no value (its _na = 1) with R = 1 or a minimum of 0.  The verdict, decided in integers as max <
 *   2 * min: GX_REPRO_PASS both ratios below 2, GX_REPRO_BORDERLINE exactly one, GX_REPRO_FAIL neither, GX_REPRO_NA a ratio
 *   without a value.  conservative[n_run]: the run's peaks counted in Nt (none with R = 1); optimal[n_run]: the larger of that
 *   set and Np's (a tie: the conservative set).  in_run[3 R + 2]: the call's peaks supported by the run's; run_supported: the
 *   run's peaks supported by the call's.  in_run, run_supported, conservative and optimal may be NULL, nt_pair with R = 1.
 * gx_reproducibility_label: "t<rep>", "t<rep>.pr<half>", "pooled.pr<half>", replicates and halves counted from 1.
 * gx_format_reproducibility: a comment line "# run: <n> peaks, <bp> bp; overlap <pct> %; seed <seed>", then a TSV, header "call
 *   rep half intervals peaks peak_bp in_run run_supported status", one row per call; rep and half from 1, NA where the call
 *   has none; status "ok" or, for GX_ERR_EXPT, "no_fragments" (another status: its number).
 * gx_format_reproducibility_metrics: "figure value" rows: replicates, Nt.t<i>.t<j> per pair, Nt, Np, N_self.t<r>, rescue_ratio,
 *   self_consistency_ratio (%.6f or NA), verdict, conservative_peaks, optimal_peaks (Nt and conservative_peaks: NA with R = 1).
 * gx_format_narrowpeak: gx_write_narrowpeak_group's lines for a list; peak i is named peak_<first_index + i>.
 * gx_write_reproducibility (gx_api.hip: it reads a context): the last gx_reproducibility against the run's own peaks; either
 *   file may be NULL, not both. */
#define GX_REPRO_PASS 0
#define GX_REPRO_BORDERLINE 1
#define GX_REPRO_FAIL 2
#define GX_REPRO_NA 3
typedef struct { int32_t n_rep, best_i, best_j, verdict, rescue_na, self_na, optimal_is_pooled, reserved;
                 uint64_t nt, np, n_self_max, n_self_min, n_conservative, n_optimal;
                 double rescue, self_consistency; } gx_repro_figures;
int gx_peaks_supported(const gx_peak* a, size_t n_a, const gx_peak* b, size_t n_b, int pct, uint8_t* hit);
int gx_reproducibility_figures(const gx_peak* run, size_t n_run, int n_rep, const gx_repro_call* calls, const gx_peak* const* peaks,
                               int pct, gx_repro_figures* fig, uint64_t* nt_pair, uint64_t* n_self, uint64_t* in_run,
                               uint64_t* run_supported, uint8_t* conservative, uint8_t* optimal);
int gx_reproducibility_label(const gx_repro_call* call, char* out, size_t cap);
int gx_format_reproducibility(FILE* out, int n_rep, const gx_repro_call* calls, const uint64_t* in_run, const uint64_t* run_supported,
                              uint64_t n_run, uint64_t run_bp, int pct, uint64_t seed);
int gx_format_reproducibility_metrics(FILE* out, const gx_repro_figures* fig, const uint64_t* nt_pair, const uint64_t* n_self);
int gx_format_narrowpeak(const gx_peak* peaks, size_t n, const char* const* names, int first_index, FILE* out);
int gx_write_reproducibility(gx_ctx* ctx, int pct, FILE* calls_file, FILE* metrics_file);
int gx_write_pile_path(gx_ctx* ctx, int rep, const char* const* names, int n_chrom, const char* expt_name,
                       const char* ctrl_name, const char* path, int append);
int gx_write_log_path(gx_ctx* ctx, int n_rep, const char* const* names, int n_chrom, int qval_opt, int peaks_opt,
                      float thr, const char* path);

/* ---- multi-GPU hooks: chromosomes are sharded across ranks; the
 *      three genome-wide quantities are exchanged through host-supplied callbacks
 *      (RCCL via torch.distributed in bench.py; a no-op on one GPU). ---- */

/* Sum `n` int64 values over all ranks in place.  EVERY exchange of the library goes through this one callback in the
 * callback mode: the fragLen / ctrlFrag fixed-point parts and the ranks' flags (n = 3, twice per sample when lambda is
 * exchanged ahead of the tile stage), the dense p-value histogram of a run without a control (n = 2^18 + 8,194 per
 * rank), and -- as sums of disjoint regions of a zeroed buffer, i.e. concatenations -- the samples, counts, totals,
 * minima and the all-to-all segments of the range-partitioned BH exchange (gx_bhx.h).  buf is host memory. */
typedef int (*gx_allreduce_i64_fn)(int64_t* buf, size_t n, void* user);
/* (Rounds 1-5 also took a table all-gather callback here; the BH table travels by all-reduces since round 4, and round 6
 * dropped the parameter.) */
int gx_set_collectives(gx_ctx* ctx, int rank, int world, gx_allreduce_i64_fn allreduce, void* user);
/* The library's own collectives: RCCL over xGMI on device buffers, on the library's stream (no host
 * hop in the data path).  One rank calls gx_rccl_unique_id and hands the 128 bytes to every rank
 * by whatever channel the host program has; then every rank calls gx_set_rccl (collective: it
 * returns when all `world` ranks have called it).  Replaces gx_set_collectives' callbacks, which stay
 * for host programs without RCCL (the tests' gloo mode).  librccl is opened at run time. */
int gx_rccl_unique_id(void* out, size_t cap /* >= 128 */);
int gx_set_rccl(gx_ctx* ctx, int rank, int world, const void* unique_id);
/* Ranks of the library's communicator as RCCL itself reports them (ncclCommCount); 0 without one. */
int gx_rccl_nranks(gx_ctx* ctx, int* n);
/* owned[i] = 1: this rank computes chromosome i (default: all).  The full table still goes to
 * gx_set_chroms on every rank, so genome lengths and output order are global; device work and
 * memory are laid out for the owned chromosomes only.  Call after gx_set_chroms and before the
 * first gx_sample_begin (or right after gx_reset): GX_ERR_ORDER otherwise. */
int gx_set_owned(gx_ctx* ctx, const uint8_t* owned);

/* keep = 0: the treatment / control pileup floats of the p-value intervals are not written to
 * device memory (they are only ever read by gx_get_intervals, i.e. by the -f / -k emitters, which
 * then fail with GX_ERR_ORDER); interval ends, p and q are unaffected.  Default 1.  The reference
 * always keeps them (Pileup arrays, Genrich.h:208-214) and prints them only with -f / -k. */
int gx_set_keep_pileups(gx_ctx* ctx, int keep);

/* ---- introspection used by bench.py / tests ---- */

/* Per-phase device times (ms, HIP events on the library's stream) of the last
 * gx_* call sequence; names are NUL-separated in *names. Returns count.
 * gx_set_phase_timing chooses what is timed: 0 nothing (default: an event record costs a
 * ~5 us bubble on the stream), 1 the tile stage only ("t.tile" / "c.tile": what
 * bench.py's roofline needs inside its timed region), 2 every phase.
 * Independently of the level, a context made with GX_ROCTX=1 in the environment (or gx_set_knob) brackets every phase
 * with a roctx range of the phase's name ("gx:t.tile", ...) on the calling thread, so that a rocprofv3 --marker-trace
 * --kernel-trace run attributes every kernel to its phase (tools/make_counters_json.py; host-side markers, no stream
 * bubble; the roctx library is opened at run time and its absence is not an error). */
int gx_set_phase_timing(gx_ctx* ctx, int level);
/* Like level 1, for another phase: only the phases called `name` ("sort1", "tile", "bucket", "cover", "profile" -- per sample, reported
 * as "t.<name>" / "c.<name>" --, "pval", "merge", "fisher", "bh", "sweep") are bracketed by events.  bench.py times
 * the phase of its roofline kernel this way inside the timed region. */
int gx_set_phase_filter(gx_ctx* ctx, const char* name);
int gx_phase_times(gx_ctx* ctx, const char** names, const float** ms);
/* A hint, before the first sample: the run may hold fractional weights (count > 1: Genrich's -s).  The device path then
 * writes its pair records with a weight class from the start; without the hint the first sample that shows a fractional
 * weight is built a second time, on the general chain (same results either way). */
int gx_expect_fractional(gx_ctx* ctx, int on);
/* Test and measurement switches (the GX_* names of DESIGN.md's knob table: GX_NO_FUSED, GX_NO_LOOSE, GX_SBSHIFT, ...).  The
 * library reads them from the environment once, in gx_create; this sets one on a live context (bench.py times the
 * "materialised" step that way).  value: a number as text; NULL or "" = 1.  An unknown name is GX_ERR_ORDER.  Not part of
 * what a host program needs: every switch only forces a path that the default run chooses by itself. */
int gx_set_knob(gx_ctx* ctx, const char* name, const char* value);
/* Which device path the last calls took (tests assert that the fast paths really run):
 * bit 0: the last sample's tile stage was k_sbtile (level 2 of the sort fused with the tile passes, gx_sbtile.h);
 * bit 1: the last gx_find_peaks swept the tile stage's loose slots (no k_pack_pval, gx_kernels.h LooseCtl);
 * bit 2: a sample of this context was sent back to the general chain (a super-bucket beyond k_sbtile's LDS, or
 *        fractional weights);
 * bit 3: a sample of this context was built again with larger page tables (reads piled up in one super-bucket
 *        beyond what a row of the level-1 page table held). */
#define GX_PATH_FUSED 1u
#define GX_PATH_LOOSE_SWEEP 2u
#define GX_PATH_FELL_BACK 4u
#define GX_PATH_PT_GREW 8u
#define GX_PATH_PAIRS 16u    /* bit 4: level 1 of the sort wrote one record per fragment (k_sort_a / k_sort_b) for the fused kernel */
#define GX_PATH_RANGE_BH 64u /* bit 6: several ranks with a control / replicates, -q: the range-partitioned BH exchange */
#define GX_PATH_DENSE_BH 32u /* bit 5: several ranks, no control, -q: the p-value histogram travelled as ONE dense all-reduce */
#define GX_PATH_PILES_MADE 256u /* bit 8: pileup floats (Pileup.cov, printed by -f / -k only) were written since the last gx_reset */
#define GX_PATH_PACKED 512u  /* bit 9: the last sample's level 1 read 8-byte events in place (k_sort_a<.., PACKED>: gx_push_events_packed) */
#define GX_PATH_PACK_HIST 2048u /* bit 11: -q on one replicate without control: BH's table was made of the "bp at pileup V" sums that the tight table's kernel left (k_pack_pval<.., HIST>), not by k_bh_hist */
#define GX_PATH_LAZY_Q 8192u /* bit 13: -q: the sweep's significance bits came from one compare per interval against the smallest significant p, q was looked up inside the candidates only (k_sig_from_p + k_q_fill_cands; the whole q array on request) */
#define GX_PATH_LATE_LOOSE 16384u /* bit 14: ... GX_PATH_LOOSE_SWEEP on a sample whose lambda came with its end (fractional weights): the bits and the fillers were written after the tile stage (k_loose_late) */
#define GX_PATH_Q_LOOSE 32768u /* bit 15: -q on one replicate without control: no tight table -- BH's histogram from the loose slots, q by pileup, the sweep on the loose slots (k_bh_small, k_loose_late, k_peak_both<.., PVQ>) */
#define GX_PATH_MERGE_P 1024u /* bit 10: the last control merge scored its intervals itself and left (end, p) in its loose slots (k_merge2<.., true> + k_pack_ep2) */
#define GX_PATH_COUNTS 65536u /* bit 16: this run kept its samples' intervals for counting (gx_set_count_in_peaks) */
#define GX_PATH_REGION_COUNTS 131072u /* bit 17: gx_count_in_regions has counted the kept samples in a region set since the last gx_reset */
#define GX_PATH_COVERAGE 262144u /* bit 18: this run summed its samples' pileups over bins (gx_set_coverage_bins; a sample was closed since the last gx_reset) */
#define GX_PATH_PROFILE 524288u /* bit 19: this run summed its samples' pileups around anchors (gx_set_profile; a sample was closed with it on since the last gx_reset) */
#define GX_PATH_GRAM 1048576u /* bit 20: k_gram / k_gram_sum ran since the last gx_reset (gx_coverage_gram, gx_gram_u64) */
#define GX_PATH_FINGERPRINT 2097152u /* bit 21: k_fp_hist ran since the last gx_reset (gx_coverage_fingerprint, gx_fp_u64) */
#define GX_PATH_SPEARMAN 4194304u /* bit 22: k_rank ran since the last gx_reset (gx_coverage_rank_gram, gx_rank_u64) */
#define GX_PATH_COMPLEXITY 8388608u /* bit 23: k_cpx_insert ran since the last gx_reset (gx_complexity, gx_complexity_events) */
#define GX_PATH_SATURATION 16777216u /* bit 24: k_sub_write ran since the last gx_reset (gx_subsample_events, gx_subsample_kept, gx_saturation) */
#define GX_PATH_DEPTH 33554432u /* bit 25: k_depth_hist ran since the last gx_reset (gx_set_depth_hist; a sample was closed with it on) */
#define GX_PATH_IVSTAT 67108864u /* bit 26: k_ivstat ran since the last gx_reset (gx_interval_stats, gx_interval_stats_events) */
#define GX_PATH_XCOR 134217728u /* bit 27: k_xc_set / k_xc_corr ran since the last gx_reset (gx_set_xcor with a sample closed, gx_push_tags, gx_xcor_tags) */
#define GX_PATH_SPLIT 268435456u /* bit 28: k_sub_split ran since the last gx_reset (gx_subsample_split_events, gx_subsample_split_kept, gx_reproducibility) */
#define GX_PATH_SWEEP_OVERLAP 536870912u /* bit 29: ... GX_PATH_LOOSE_SWEEP whose run pass rode in the launch that scanned the tiles and closed the sample (k_scan_iv_close_runs), ahead of gx_find_peaks: the sweep launched no k_runs */
#define GX_PATH_GC 1073741824u /* bit 30: a kernel of the genome / GC passes ran since the last gx_reset (gx_push_sequence, gx_genome_info, gx_gc_content, gx_gc_bias, gx_gc_bias_events) */
#define GX_PATH_MOTIFS 2147483648u /* bit 31: k_motif_scan ran since the last gx_reset (gx_motif_scan_regions, gx_motif_scan_peaks, gx_motif_scan_genome) */
#define GX_PATH_KMERS 4096u /* bit 12: k_kmer_count ran since the last gx_reset (gx_kmer_count_regions, gx_kmer_count_peaks, gx_kmer_count_genome) */
#define GX_PATH_FRAC_PAIRS 128u /* bit 7: ... and the pair records carried a weight class (k_sort_a<FRAC> / k_sbtile<.., FRAC>: -s multimapping) */
int gx_path_info(gx_ctx* ctx, unsigned* flags);

/* Evaluate one scalar device function on n inputs (numerics tests):
 * what 0: log10f as the host libm computes it (saveQval 221/226)   out = f(a)
 *      1: calcPval(expt = a, ctrl = b)          (Genrich.c:1628)
 *      2: getVal of the exact pileup whose int32 bits are in a (1/120 units, :1902)
 *      3: multPval's combination of sum = a over df = b (567-583), by the reference's own algorithm (pgamma's series)
 *      4: the same by the closed form of the even-df tail that the merge kernels evaluate (gx_math.h fisher_fast); a value next
 *         to a float rounding boundary is re-evaluated by 3's algorithm on the host, like everywhere */
int gx_selftest(gx_ctx* ctx, int what, const float* a, const float* b, float* out, size_t n);
/* The same, plus (what 1 and 3) the double each result was rounded from in out_double (may be NULL)
 * and the number of results that lay next to a float rounding boundary and were therefore
 * re-evaluated with the host's libm ("risky", gx_math.h) in *n_risky (may be NULL). */
int gx_selftest2(gx_ctx* ctx, int what, const float* a, const float* b, float* out, double* out_double,
                 size_t n, size_t* n_risky);
/* what 1, 3 and 4 evaluated by the host build of the same routines (this machine's libm, as the
 * reference would call it); no context and no device needed. */
int gx_selftest_host(int what, const float* a, const float* b, float* out, double* out_double, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* GENRICH_AMD_H */
