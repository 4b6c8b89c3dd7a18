// genrich_amd.cpp -- host program: the Genrich command line over the MI355X hot path.
//
// Everything upstream of the C ABI stays on the CPU, as north_star prescribes: option handling
// (getArgs, Genrich.c:5718-5827), SAM / BAM reading (readSAM 4468, readBAM 4983), pairing of
// alignments into fragments (parseAlign 4141, processAlns 3187), multimap weighting
// (processPair 3122, processSingle 3019), interval geometry (saveFragment 2754, saveFragAtac
// 2728, saveUnpair 2689, processAvgExt 2614) and saveInterval's clamping / -b line (2516-2591).
// Each alignment-derived interval becomes one gx_event; pileups, p/q-values and peaks come
// from libgenrich_amd.so; text output is gx_emit.cpp.  Written from the behaviour described in
// SURVEY.md Appendix A, not transliterated from the reference.
//
// -P (peak calling from a -f log, callPeaksLog 1277-1488) is text processing and runs on the host,
// and so does -r / -R (PCR-duplicate removal, Genrich.c:2776-2977 and 3267-4042).
//
// Extra long options:
//   --threads N     threads that inflate BGZF (BAM, bgzip-ped SAM) input, as many that decode records (SAM lines,
//                   BAM blocks: everything that does not touch the run's state) and as many that run the pairing /
//                   weighting state machine over chunks of whole read-name groups (results merged in file order);
//                   default min(16, cores); 1: one thread does it all, in the reference's order of operations
//   (environment, for tests: GENRICH_BATCH_BYTES, GENRICH_CHUNK_RECS -- where the input is cut; GENRICH_SERIAL_STATE=1 --
//   one thread for the state machine)
//   (environment: GENRICH_HOST_PROF=1 prints the CPU time of the parsing thread after the last input; GENRICH_DUPS_HOST=1
//   keeps -r's tables on the host; GENRICH_NO_INT16=1 leaves saveInterval's int16 checks to the library -- the pileup is the
//   reference's either way, the -v warnings / -b lines / -x average of dropped reads only with the checks on; GENRICH_NO_MMAP=1
//   reads plain files through read() instead of mapping them; GENRICH_ZLIB_INFLATE=1 inflates BGZF blocks with zlib instead of
//   gx_inflate.h; GENRICH_THREADS_REPORT=1 prints how the thread budget was split)
//   --events-only   parse and write the -b file without touching a GPU (diagnostics)
//   --device N      HIP device ordinal (default 0)
//   --devices LIST  several GPUs of one node, e.g. 0-7 or 0,2,5: chromosomes are sharded over them by length, one
//                   library context and one host thread per GPU, RCCL inside the library for the two genome-wide
//                   exchanges, outputs identical to a single-GPU run (a device named twice, e.g. 0,0, runs the
//                   same protocol through host callbacks: the test mode for a single GPU)
#include <getopt.h>
#include <zlib.h>

#include <cctype>
#include <chrono>
#include <cerrno>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <pthread.h>
#include <unistd.h>
#include <thread>
#include <vector>

#include "../../include/genrich_amd.h"
#include "bgzf_reader.h"
#include "../csrc/gx_saturate.h"  // (host-only: the canonical int16 part of a difference, the weights)

#define VERSION "0.6.2-amd"
#define MAX_ALNS 128  // Genrich.h:17 (also the length of stored read names)
static const float NOSCORE = -FLT_MAX;

// the program by stage, one translation unit; this file keeps the thread budget, the usage texts and main
#include "host_motifs.h"   // --motifs: the JASPAR reader
#include "host_common.h"   // die, number parsing, output files, the input stream
#include "host_state.h"    // options, chromosome table, device contexts, HotWindows
#include "host_events.h"   // the alignments of a read name -> events (pairing, weighting, saveInterval)
#include "host_dups.h"     // -r / -R
#include "host_ingest.h"   // SAM / BAM decoding, the decode pipeline, the parallel state workers
#include "host_peaklog.h"  // -P
#include "host_genome.h"   // --genome: the FASTA reader
#include "host_figures.h"  // --counts ... --profile: the writers, and FIGURES, the table of them

namespace {

// --threads N (else GENRICH_THREADS, else up to 16 of the machine's cores) sizes three pools next to the reader and the owner: on a
// host with fewer than 3 N + 2 cores the pools share the budget instead of each taking N (inflate N / 4, decode N / 2, state
// workers N / 2: the stages' measured shares of the work)
Threads splitThreads(int n) {
  Threads T;
  T.sam = T.bam = ThreadSplit{n, n, n};
  const unsigned hw = std::thread::hardware_concurrency();
  if (hw && (unsigned)(3 * n + 2) > hw && n > 2) {
    T.sam = ThreadSplit{std::max(2, n / 4), std::max(2, n / 2), std::max(1, n / 2)};   // (two inflaters keep the BGZF reader with its block checks)
    T.bam = ThreadSplit{std::max(2, n / 2), std::max(2, n / 4), std::max(1, n / 4)};
  } else if (hw && n > 1) {
    // cores to spare: a BAM stream gets twice the inflaters (the other pools keep up with 40 M records/s of SAM text)
    T.bam.inflate = std::min(2 * n, std::max(n, (int)hw - 2 * n - 2));
  }
  if (getenv("GENRICH_THREADS_REPORT"))
    fprintf(stderr, "[threads] inflate %d, decode %d, state %d; BAM: inflate %d, decode %d, state %d\n", T.sam.inflate, T.sam.decode, T.sam.state,
            T.bam.inflate, T.bam.decode, T.bam.state);
  return T;
}

[[noreturn]] void usage() {
  fprintf(stderr,
          "Usage: genrich-amd  -t <file>  -o <file>  [optional arguments]\n"
          "  (same options as Genrich v0.6.2: -t -c -o -f -k -b -z -y -w -x -j -d -D -e -E -m -s\n"
          "   -r -R -p -q -a -l -g -X -P -S -L -v -V)\n"
          "  --device N | --devices 0-7   GPU(s) to use;  --threads N   BGZF inflate threads\n"
          "  --counts FILE   each sample's intervals counted in the called peaks\n"
          "  --peak-signal FILE   each sample's own depth inside the called peaks: max, summit, area, covered bases, depth at the summit\n"
          "  --count-regions BED --region-counts FILE   ... counted in the BED's regions, one row per BED line\n"
          "  --coverage PREFIX [--bin-size N] [--coverage-scale X]   each sample's pileup in bins of N bases (50):\n"
          "                  bedGraph PREFIX.t<rep>.bedgraph / PREFIX.c<rep>.bedgraph, values times X (1)\n"
          "  --correlation FILE [--corr-skip-zeros]   the samples' Pearson correlation matrix over their bins of --bin-size N (50)\n"
          "                  bases, a TSV labelled t<rep> / c<rep>; --corr-skip-zeros leaves out the bins that are 0 in every sample\n"
          "  --spearman FILE [--corr-skip-zeros]   the samples' Spearman correlation matrix over their bins of --bin-size N (50)\n"
          "                  bases, a TSV labelled t<rep> / c<rep>; --corr-skip-zeros leaves out the bins that are 0 in every sample\n"
          "                  before they are ranked\n"
          "  --fingerprint FILE [--fingerprint-metrics FILE]   each sample's fingerprint (Lorenz curve) over its bins of --bin-size N (50)\n"
          "                  bases: a TSV of cumulative bins and signal per value class; the metrics file has the zero fraction, area,\n"
          "                  Gini, elbow and the divergence from the replicate's control per sample\n"
          "  --complexity FILE [--complexity-hist FILE]   each sample's library complexity from its intervals (the -b lines) as\n"
          "                  (chromosome, start, end) keys: N, distinct, NRF, PBC1, PBC2, duplicate fraction, estimated library size and\n"
          "                  the expected distinct keys at 5 %% .. 100 %% of the depth, a TSV labelled t<rep> / c<rep>; the histogram\n"
          "                  file has the number of keys seen m times per sample and m\n"
          "  --lengths FILE [--lengths-metrics FILE] [--lengths-cuts A,B,...] [--chrom-stats FILE]   each sample's intervals (the -b\n"
          "                  lines) by length: a TSV labelled t<rep> / c<rep> with the intervals, their weight and the cumulative share of\n"
          "                  the weight at every length that occurs; the metrics file has the mean, sd, min, p5, quartiles, p95, max, mode\n"
          "                  and the shares of weight below A, from A to B, ... (150,300,500; at most 8 ascending positive integers); the\n"
          "                  chrom-stats file has one row per chromosome with each sample's intervals, weight, share and mean depth (a\n"
          "                  chromosome skipped with -e: zeros); each of the three files may stand alone; with -j the intervals are\n"
          "                  cut-site windows, nearly all of one length, not fragments; not with -P or --events-only\n"
          "  --xcor FILE [--xcor-metrics FILE] [--xcor-shifts LO,HI] [--xcor-read-length R] [--xcor-unpaired]   each sample's strand\n"
          "                  cross-correlation: a forward alignment tags its first base on the plus strand, a reverse one its last base\n"
          "                  on the minus strand, a proper pair both ends of its fragment (--xcor-unpaired: unpaired alignments only);\n"
          "                  positions, not reads, are counted (duplicates count once, -s weights not at all).  The curve is a TSV\n"
          "                  labelled t<rep> / c<rep> with, per shift LO .. HI (-100,600; within -4096 .. 4096), the positions tagged on\n"
          "                  the plus strand with a minus tag that far downstream and the correlation r; the metrics file (it may stand\n"
          "                  alone) has the fragment length (1 + the shift >= 1 of the greatest r), NSC = r there over the least r, and\n"
          "                  with the read length R the phantom peak at R - 1 (shifts within 10 of it are then no fragment peak) and\n"
          "                  RSC; with -v and a library of unpaired alignments the length to extend them to; not with -P or --events-only\n"
          "  --depth FILE [--depth-metrics FILE]   each sample's distribution of per-base depth over every base of the genome outside\n"
          "                  the -E regions: a TSV labelled t<rep> / c<rep> with the bases at each whole depth and at that depth or\n"
          "                  more; the metrics file (it may stand alone) has the bases, the share covered, mean, sd, min, quartiles,\n"
          "                  p95, p99, max and the shares at 1x, 2x, 5x, 10x, 20x, 50x, 100x per sample\n"
          "  --saturation FILE [--saturation-steps N] [--saturation-seed S] [--saturation-controls]   the peaks called once more on\n"
          "                  N (10, at most 100) nested subsamples of the run's intervals, j / N of them for j = 1 .. N drawn with seed S\n"
          "                  (1): a TSV with one row per point -- fraction, threshold, intervals kept, peaks, peak bp, the run's peaks\n"
          "                  recovered and their share, the point's peaks that touch one of the run's, shared bp, status; the controls\n"
          "                  stay whole unless --saturation-controls; one device; not with -X, -P or --events-only\n"
          "  --profile BED --profile-out PREFIX [--flank N] [--profile-bin N] [--profile-at tss|center] [--profile-matrix]\n"
          "                  each sample's pileup around the BED's sites, N (2000) bases to either side in bins of N (10) bases,\n"
          "                  oriented by column 6: PREFIX.profile.tsv, the mean per base and site at every offset; a site is the\n"
          "                  line's 5' end (tss) or its middle (center); --profile-matrix: one row per site and sample in\n"
          "                  PREFIX.t<rep>.matrix.tsv / PREFIX.c<rep>.matrix.tsv; -v: the highest bin over the mean of the 100\n"
          "                  bases at either end -- with the defaults ENCODE's TSS enrichment, unsmoothed\n");
  exit(EXIT_FAILURE);
}

// --help-reproducibility: the block of --reproducibility and its sub-options, in usage()'s form (to the same stream, with the same
// exit status); it stands apart so that the -h text stays as recorded
[[noreturn]] void usageReproducibility() {
  fprintf(stderr,
          "  --reproducibility FILE [--reproducibility-metrics FILE] [--reproducibility-overlap PCT] [--reproducibility-seed S]\n"
          "                  [--reproducibility-peaks PREFIX]   the peaks called once more on every replicate alone, on two random\n"
          "                  halves (pseudo-replicates) of every replicate drawn with seed S (1), and on the two pools of halves,\n"
          "                  3 R + 2 calls for R replicates; the controls stay whole.  A TSV with one row per call -- t<rep>,\n"
          "                  t<rep>.pr1, t<rep>.pr2, pooled.pr1, pooled.pr2: intervals, peaks, peak bp, the call's peaks that one of the\n"
          "                  run's supports, the run's peaks that one of the call's supports, status; a peak supports another when\n"
          "                  they share at least one base and PCT %% (50; 0 .. 100) of the shorter of the two.  The metrics file (it may\n"
          "                  stand alone) has Nt per pair of replicates and the greatest, Np, N_self per replicate, the rescue and\n"
          "                  self-consistency ratios, the verdict (pass, borderline, fail, NA) and the sizes of the conservative and\n"
          "                  optimal sets; --reproducibility-peaks writes PREFIX.<call>.narrowPeak per call and the run's own -o lines\n"
          "                  of the two sets as PREFIX.conservative.narrowPeak and PREFIX.optimal.narrowPeak; one device; not with -X,\n"
          "                  -P or --events-only\n");
  exit(EXIT_FAILURE);
}

// --help-summits: the block of --summits and its sub-options, likewise
[[noreturn]] void usageSummits() {
  fprintf(stderr,
          "  --summits FILE [--summits-prominence PCT] [--summits-height PCT]   the local maxima of the treatments' pooled depth\n"
          "                  (controls never; -E regions not masked) inside every called peak: a TSV, BED in its first six columns,\n"
          "                  one row per summit -- chr, summit, summit + 1, peak_N.j (j = 1, 2, ... from left to right in peak_N of\n"
          "                  -o), height, ., the plateau's start and end, prominence, the peak's start and end.  A plateau of equal\n"
          "                  depth is a maximum when the depth is lower on both sides; the summit is its middle.  The prominence is\n"
          "                  the height over the higher of the two lowest depths between the plateau and the nearest higher base (or\n"
          "                  the peak's end) on either side.  The highest maximum of a peak is always reported, every other one\n"
          "                  whose prominence is at least PCT %% (25; 0 .. 100) of its height and whose height is at least PCT %% (50;\n"
          "                  0 .. 100) of the peak's highest; -v: the peaks with more than one summit; not with -X, -P or --events-only\n");
  exit(EXIT_FAILURE);
}

// --help-gc: the block of --genome, --gc-bias and --gc-peaks, likewise
[[noreturn]] void usageGc() {
  fprintf(stderr,
          "  --genome FASTA  the reference sequence the alignments were made against: plain text (any line width, CRLF, lower\n"
          "                  case; N and the IUPAC codes are unknown bases) or gzip / BGZF; it goes to the device as two bits per\n"
          "                  base.  A sequence the alignment files' headers do not name is skipped; one whose length differs from\n"
          "                  its LN ends the run; a chromosome that is missing stays unknown (-v says so).  With --devices each\n"
          "                  sequence goes to the device that owns its chromosome.  Needs --gc-bias or --gc-peaks\n"
          "  --gc-bias FILE [--gc-window W]   each sample's GC bias (the fragment model of Benjamini & Speed, deepTools'\n"
          "                  computeGCBias): every interval (-b line) is classed by the G + C among the W (200; 1 .. 4096) bases\n"
          "                  from its start, whatever its own length, and so is EVERY window of the genome, not a sample of them;\n"
          "                  a window with an unknown base, or one that runs past its chromosome, is not classed.  A TSV labelled\n"
          "                  t<rep> / c<rep>: per sample a # line (W, the classed and unclassed windows and intervals), then per GC\n"
          "                  percent 0 .. 100 the genome's windows, the sample's intervals, their weight and the ratio of the two\n"
          "                  shares (NA where the genome has no such window).  -E regions are NOT masked on either side; -v: the\n"
          "                  mean window GC of the sample and of the genome, the least and the greatest ratio among the classes\n"
          "                  with 1 %% of the windows; works with -X, -z, -r, --devices; not with -P or --events-only\n"
          "  --gc-peaks FILE the rows of --counts (chr, start, end, peak_N), then the peak's length, its known bases, the G + C\n"
          "                  among them and their share (NA without known bases); needs --genome only; not with -X, -P (no\n"
          "                  device context exists there) or --events-only\n");
  exit(EXIT_FAILURE);
}

// --help-motifs: the block of --motifs and its sub-options, likewise
[[noreturn]] void usageMotifs() {
  fprintf(stderr,
          "  --motifs FILE   known motifs as JASPAR count matrices (`>ID NAME`, then four rows `A [ n n ... ]` .. `T [ ... ]`, or four\n"
          "                  bare rows in the order A C G T; widths 1 .. 32, at most 4096 motifs), scanned on the device at every\n"
          "                  position of every called peak on both strands.  Scores are log-odds against a uniform background in\n"
          "                  1/128 bit; a motif's threshold is the least score that at most a share P of all 4^L L-mers reach,\n"
          "                  counted exactly.  A window with an unknown base is not scanned; -E regions are NOT masked.  Needs\n"
          "                  --genome FASTA and --motif-hits or --motif-summary; works with -z, --devices; not with -X, -P or\n"
          "                  --events-only\n"
          "  --motif-hits FILE   one BED-like row per hit in the order of -o, then position, motif, strand: chr, start, end, ID,\n"
          "                  score (bits), strand, NAME, peak_N, the offset of the window's middle from the peak's summit and the\n"
          "                  threshold's p\n"
          "  --motif-summary FILE   one row per motif: ID, NAME, width, threshold (bits) and its p, the peaks long enough to scan and\n"
          "                  those with a hit, the windows and hits (both strands) in the peaks and in the WHOLE genome (every\n"
          "                  window of every chromosome that takes part, counted, not sampled) and the enrichment (hits per window in\n"
          "                  the peaks over hits per window in the genome; NA without a hit in the genome)\n"
          "  --motif-pvalue P (1e-4; 0 < P <= 1), --motif-pseudocount X (1; added to each column, a quarter to each base)\n"
          "                  -v: the motifs read, those that cannot hit at P, the hits, the peaks with any, the three most enriched\n"
          "                  motifs and the time of the genome pass\n");
  exit(EXIT_FAILURE);
}

// --help-kmers: the block of --kmers and its sub-options, likewise
[[noreturn]] void usageKmers() {
  fprintf(stderr,
          "  --kmers FILE [--kmer-k K] [--kmer-flank N] [--kmer-top N]   the K-mers (8; 1 .. 12) that are over-represented in the\n"
          "                  called peaks: every window of K known bases of every peak -- whole, or with --kmer-flank the N bases to\n"
          "                  either side of its summit -- counted on the device, and every window of the WHOLE genome (every\n"
          "                  chromosome that takes part; counted, not sampled or shuffled) as the background.  A K-mer and its\n"
          "                  reverse complement are one row (the smaller of the two names it; a palindrome counts once).  A TSV: a #\n"
          "                  line (k, flank, the regions counted, the windows of the peaks and of the genome, the K-mers counted in\n"
          "                  the peaks), then kmer, revcomp, count_peaks, count_genome, enrichment (the peaks' share over the\n"
          "                  genome's) and z, the binomial z-score of count_peaks among the peaks' windows at the genome's rate; the\n"
          "                  N (100; 0: all) rows of highest z.  Overlapping windows are not independent: z ranks K-mers, it is not a\n"
          "                  p-value.  A window with an unknown base is not counted; overlapping regions count twice; -E regions\n"
          "                  are NOT masked.  Needs --genome FASTA; works with -z, --devices and next to every other output; not\n"
          "                  with -X, -P or --events-only; -v: the windows, the three top K-mers and the genome pass's seconds\n");
  exit(EXIT_FAILURE);
}

}  // namespace

#include "host_options.h"  // the table of long options, parseOptions (behind the thread budget and the usage texts, which they call)
#include "host_run.h"      // validate ... writeOutputs: the stages main calls

int main(int argc, char** argv) {
  State S;
  const Opts& o = S.o;
  parseOptions(argc, argv, S.o);
  planSamples(S);   // (before validate, which counts the samples; it reads and prints nothing)
  validate(S);
  loadRegionInputs(S);
  if (o.peaksOnly) {  // runProgram 5398-5403
    peaksOnly(S, S.thr);
    return EXIT_SUCCESS;
  }
  openStreams(S);
  if (!o.eventsOnly) {
    createContexts(S);
    joinDevices(S);
  }
  scanHeaders(S);
  enablePasses(S);
  // loop over the comma-separated treatment / control lists (runProgram 5455-5585)
  for (size_t r = 0; r < S.tFiles.size(); r++) {
    for (auto& ch : S.chrom) ch.save = false;
    readSampleFile(S, S.tFiles[r].c_str(), false);
    closeSample(S, false);
    if (S.controlOf(r)) {
      readSampleFile(S, S.controlOf(r), true);
      closeSample(S, true);
    } else
      noControl(S);
    if (S.gx) onEachDevice(S, [&](int g) { return gx_pvalues(S.devs.ctx[g]); });
    S.sample++;
  }
  closeStreams(S);
  if (o.eventsOnly) return EXIT_SUCCESS;
  callPeaks(S);
  writeOutputs(S);
  for (gx_ctx* g : S.devs.ctx) gx_destroy(g);
  return EXIT_SUCCESS;
}
