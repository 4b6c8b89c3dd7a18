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

// the program by stage, one translation unit; this file keeps the thread budget, usage(), the options and main
#include "host_motifs.h"   // --motifs: the JASPAR reader
#include "host_common.h"   // die, number parsing, output files, the input stream
#include "host_state.h"    // options, chromosome table, device contexts, HotWindows
#include "host_events.h"   // the alignments of a read name -> events (pairing, weighting, saveInterval)
#include "host_dups.h"     // -r / -R
#include "host_ingest.h"   // SAM / BAM decoding, the decode pipeline, the parallel state workers
#include "host_peaklog.h"  // -P
#include "host_genome.h"   // --genome: the FASTA reader
#include "host_figures.h"  // --counts ... --profile

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

void usage() {
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
void usageReproducibility() {
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
void usageSummits() {
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
void usageGc() {
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
void usageMotifs() {
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

}  // namespace

int main(int argc, char** argv) {
  State S;
  Opts& o = S.o;
  static struct option longOpts[] = {{"help", no_argument, nullptr, 'h'},
                                     {"verbose", no_argument, nullptr, 'v'},
                                     {"version", no_argument, nullptr, 'V'},
                                     {"events-only", no_argument, nullptr, 1000},
                                     {"device", required_argument, nullptr, 1001},
                                     {"devices", required_argument, nullptr, 1003},
                                     {"threads", required_argument, nullptr, 1002},
                                     {"counts", required_argument, nullptr, 1004},
                                     {"peak-signal", required_argument, nullptr, 1029},
                                     {"count-regions", required_argument, nullptr, 1005},
                                     {"region-counts", required_argument, nullptr, 1006},
                                     {"coverage", required_argument, nullptr, 1007},
                                     {"bin-size", required_argument, nullptr, 1008},
                                     {"coverage-scale", required_argument, nullptr, 1009},
                                     {"profile", required_argument, nullptr, 1010},
                                     {"profile-out", required_argument, nullptr, 1011},
                                     {"flank", required_argument, nullptr, 1012},
                                     {"profile-bin", required_argument, nullptr, 1013},
                                     {"profile-at", required_argument, nullptr, 1014},
                                     {"profile-matrix", no_argument, nullptr, 1015},
                                     {"correlation", required_argument, nullptr, 1016},
                                     {"corr-skip-zeros", no_argument, nullptr, 1017},
                                     {"fingerprint", required_argument, nullptr, 1018},
                                     {"fingerprint-metrics", required_argument, nullptr, 1019},
                                     {"spearman", required_argument, nullptr, 1020},
                                     {"complexity", required_argument, nullptr, 1021},
                                     {"complexity-hist", required_argument, nullptr, 1022},
                                     {"saturation", required_argument, nullptr, 1023},
                                     {"saturation-steps", required_argument, nullptr, 1024},
                                     {"saturation-seed", required_argument, nullptr, 1025},
                                     {"saturation-controls", no_argument, nullptr, 1026},
                                     {"depth", required_argument, nullptr, 1027},
                                     {"depth-metrics", required_argument, nullptr, 1028},
                                     {"xcor", required_argument, nullptr, 1034},
                                     {"xcor-metrics", required_argument, nullptr, 1035},
                                     {"xcor-shifts", required_argument, nullptr, 1036},
                                     {"xcor-read-length", required_argument, nullptr, 1037},
                                     {"xcor-unpaired", no_argument, nullptr, 1038},
                                     {"lengths", required_argument, nullptr, 1030},
                                     {"lengths-metrics", required_argument, nullptr, 1031},
                                     {"lengths-cuts", required_argument, nullptr, 1032},
                                     {"chrom-stats", required_argument, nullptr, 1033},
                                     {"reproducibility", required_argument, nullptr, 1039},
                                     {"reproducibility-metrics", required_argument, nullptr, 1040},
                                     {"reproducibility-overlap", required_argument, nullptr, 1041},
                                     {"reproducibility-seed", required_argument, nullptr, 1042},
                                     {"reproducibility-peaks", required_argument, nullptr, 1043},
                                     {"help-reproducibility", no_argument, nullptr, 1044},
                                     {"summits", required_argument, nullptr, 1045},
                                     {"summits-prominence", required_argument, nullptr, 1046},
                                     {"summits-height", required_argument, nullptr, 1047},
                                     {"help-summits", no_argument, nullptr, 1048},
                                     {"genome", required_argument, nullptr, 1049},
                                     {"gc-bias", required_argument, nullptr, 1050},
                                     {"gc-window", required_argument, nullptr, 1051},
                                     {"gc-peaks", required_argument, nullptr, 1052},
                                     {"help-gc", no_argument, nullptr, 1053},
                                     {"motifs", required_argument, nullptr, 1054},
                                     {"motif-hits", required_argument, nullptr, 1055},
                                     {"motif-summary", required_argument, nullptr, 1056},
                                     {"motif-pvalue", required_argument, nullptr, 1057},
                                     {"motif-pseudocount", required_argument, nullptr, 1058},
                                     {"help-motifs", no_argument, nullptr, 1059},
                                     {nullptr, 0, nullptr, 0}};
  int nThreads;  // BGZF inflate threads and record decoders: --threads N, else GENRICH_THREADS, else up to 16 of the machine's cores
  {
    const char* e = getenv("GENRICH_THREADS");
    unsigned hw = std::thread::hardware_concurrency();
    nThreads = e ? atoi(e) : (int)std::min(16u, hw ? hw : 1u);
  }
  int c;
  while ((c = getopt_long(argc, argv, "ht:c:o:f:k:b:zyw:xjd:De:E:m:s:p:q:a:l:g:rR:XPSL:vV", longOpts, nullptr)) != -1)
    switch (c) {
      case 't': o.inFile = optarg; break;
      case 'c': o.ctrlFile = optarg; break;
      case 'o': o.outFile = optarg; break;
      case 'f': o.logFile = optarg; break;
      case 'k': o.pileFile = optarg; break;
      case 'b': o.bedFile = optarg; break;
      case 'z': o.gzOut = true; break;
      case 'y': o.singleOpt = true; break;
      case 'w': o.extend = getInt(optarg); o.extendOpt = true; break;
      case 'x': o.avgExtOpt = true; break;
      case 'j': o.atacOpt = true; break;
      case 'd': o.atacLen5 = getInt(optarg); break;
      case 'D': o.atacAdj = false; break;
      case 'e': o.xchrom = optarg; break;
      case 'E': o.xFile = optarg; break;
      case 'm': o.minMapQ = getInt(optarg); break;
      case 's': o.asDiff = getFloat(optarg); break;
      case 'p': o.pqvalue = getFloat(optarg); break;
      case 'q': o.pqvalue = getFloat(optarg); o.qvalOpt = true; break;
      case 'a': o.minAUC = getFloat(optarg); break;
      case 'l': o.minLen = getInt(optarg); break;
      case 'g': o.maxGap = getInt(optarg); break;
      case 'r': o.dupsOpt = true; break;
      case 'R': o.dupsFile = optarg; break;
      case 'X': o.peaksOpt = false; break;
      case 'P': o.peaksOnly = true; break;
      case 'S': o.sortOpt = false; break;
      case 'L': o.genomeLen = (uint64_t)getLong(optarg); break;
      case 'v': o.verbose = true; break;
      case 'V': fprintf(stderr, "genrich-amd, version %s (Genrich 0.6.2 hot path on MI355X)\n", VERSION); exit(EXIT_FAILURE);
      case 1000: o.eventsOnly = true; break;
      case 1001: o.device = getInt(optarg); break;
      case 1002: nThreads = getInt(optarg); break;
      case 1004: o.countsFile = optarg; break;
      case 1029: o.peakSignalFile = optarg; break;
      case 1005: o.regionsBed = optarg; break;
      case 1006: o.regionCountsFile = optarg; break;
      case 1007: o.coveragePrefix = optarg; break;
      case 1008: o.binSize = getInt(optarg); o.binSizeOpt = true; break;
      case 1009: {  // (a double: the track's values are computed in doubles)
        char* end;
        o.coverageScale = strtod(optarg, &end);
        if (end == optarg || *end != '\0') die(optarg, ": cannot convert to float");
        o.coverageScaleOpt = true;
        break;
      }
      case 1010: o.profileBed = optarg; break;
      case 1011: o.profilePrefix = optarg; break;
      case 1012: o.flank = getInt(optarg); o.flankOpt = true; break;
      case 1013: o.profileBin = getInt(optarg); o.profileBinOpt = true; break;
      case 1014:
        if (strcmp(optarg, "tss") && strcmp(optarg, "center")) die(optarg, ": --profile-at takes tss or center");
        o.profileCenter = !strcmp(optarg, "center");
        o.profileAtOpt = true;
        break;
      case 1015: o.profileMatrix = true; break;
      case 1016: o.correlationFile = optarg; break;
      case 1017: o.corrSkipZeros = true; break;
      case 1018: o.fingerprintFile = optarg; break;
      case 1019: o.fingerprintMetricsFile = optarg; break;
      case 1021: o.complexityFile = optarg; break;
      case 1022: o.complexityHistFile = optarg; break;
      case 1027: o.depthFile = optarg; break;
      case 1028: o.depthMetricsFile = optarg; break;
      case 1034: o.xcorFile = optarg; break;
      case 1035: o.xcorMetricsFile = optarg; break;
      case 1038: o.xcorUnpaired = true; break;
      case 1036: {  // --xcor-shifts LO,HI: two integers, -4096 <= LO <= HI <= 4096
        const char* t = optarg;
        __int128 lo, hi;
        if (!strictInt(t, -GX_XCOR_MAX_SHIFT, GX_XCOR_MAX_SHIFT, &lo, &t) || !t || !strictInt(t, -GX_XCOR_MAX_SHIFT, GX_XCOR_MAX_SHIFT, &hi) || lo > hi)
          die(optarg, ": --xcor-shifts takes two integers LO,HI with -4096 <= LO <= HI <= 4096");
        o.xcorLo = (int)lo;
        o.xcorHi = (int)hi;
        o.xcorShiftsOpt = true;
        break;
      }
      case 1037: {  // --xcor-read-length R: a positive integer
        __int128 v;
        if (!strictInt(optarg, 1, 1000000, &v)) die(optarg, ": --xcor-read-length takes a positive integer (at most 1000000)");
        o.xcorReadLen = (int)v;
        break;
      }
      case 1030: o.lengthsFile = optarg; break;
      case 1031: o.lengthsMetricsFile = optarg; break;
      case 1033: o.chromStatsFile = optarg; break;
      case 1032: {  // --lengths-cuts A,B,...: at most 8 ascending positive integers
        o.lengthsCuts.clear();
        o.lengthsCutsOpt = true;
        for (const char* t = optarg; t;) {
          __int128 v;
          if (o.lengthsCuts.size() == GX_LEN_MAX_CUTS || !strictInt(t, 1, 0xffffffffll, &v, &t) || (!o.lengthsCuts.empty() && (uint64_t)v <= o.lengthsCuts.back()))
            die(optarg, ": --lengths-cuts takes at most 8 ascending positive integers, A,B,...");
          o.lengthsCuts.push_back((uint64_t)v);
        }
        break;
      }
      case 1023: o.saturationFile = optarg; break;
      case 1024: o.saturationSteps = getInt(optarg); o.saturationStepsOpt = true; break;
      case 1025: {
        __int128 v;
        if (!strictInt(optarg, 0, (__int128)UINT64_MAX, &v)) die(optarg, ": --saturation-seed takes an integer in [0, 2^64 - 1]");
        o.saturationSeed = (uint64_t)v;
        o.saturationSeedOpt = true;
        break;
      }
      case 1026: o.saturationControls = true; break;
      case 1039: o.reproFile = optarg; break;
      case 1040: o.reproMetricsFile = optarg; break;
      case 1041: {
        __int128 v;
        if (!strictInt(optarg, 0, 100, &v)) die(optarg, ": --reproducibility-overlap takes an integer in [0, 100]");
        o.reproPct = (int)v;
        o.reproPctOpt = true;
        break;
      }
      case 1042: {
        __int128 v;
        if (!strictInt(optarg, 0, (__int128)UINT64_MAX, &v)) die(optarg, ": --reproducibility-seed takes an integer in [0, 2^64 - 1]");
        o.reproSeed = (uint64_t)v;
        o.reproSeedOpt = true;
        break;
      }
      case 1043: o.reproPrefix = optarg; break;
      case 1044: usageReproducibility();
      case 1045: o.summitsFile = optarg; break;
      case 1046: {
        __int128 v;
        if (!strictInt(optarg, 0, 100, &v)) die(optarg, ": --summits-prominence takes an integer in [0, 100]");
        o.summitsProminence = (int)v;
        o.summitsProminenceOpt = true;
        break;
      }
      case 1047: {
        __int128 v;
        if (!strictInt(optarg, 0, 100, &v)) die(optarg, ": --summits-height takes an integer in [0, 100]");
        o.summitsHeight = (int)v;
        o.summitsHeightOpt = true;
        break;
      }
      case 1048: usageSummits();
      case 1049: o.genomeFile = optarg; break;
      case 1050: o.gcBiasFile = optarg; break;
      case 1051: {
        __int128 v;
        if (!strictInt(optarg, 1, GX_GC_MAX_WINDOW, &v)) die(optarg, ": --gc-window takes an integer in [1, 4096]");
        o.gcWindow = (int)v;
        o.gcWindowOpt = true;
        break;
      }
      case 1052: o.gcPeaksFile = optarg; break;
      case 1053: usageGc();
      case 1054: o.motifsFile = optarg; break;
      case 1055: o.motifHitsFile = optarg; break;
      case 1056: o.motifSummaryFile = optarg; break;
      case 1057: {
        char* end = nullptr;
        o.motifPvalue = strtod(optarg, &end);
        if (end == optarg || *end || !(o.motifPvalue > 0.0) || !(o.motifPvalue <= 1.0)) die(optarg, ": --motif-pvalue takes a number in (0, 1]");
        o.motifPvalueOpt = true;
        break;
      }
      case 1058: {
        char* end = nullptr;
        o.motifPseudo = strtod(optarg, &end);
        if (end == optarg || *end || !(o.motifPseudo >= 0.0) || !std::isfinite(o.motifPseudo)) die(optarg, ": --motif-pseudocount takes a number >= 0");
        o.motifPseudoOpt = true;
        break;
      }
      case 1059: usageMotifs();
      case 1020: o.spearmanFile = optarg; break;
      case 1003: {  // --devices 0,1,2 or 0-7
        std::string list(optarg);
        for (char* t = strtok(list.data(), ","); t; t = strtok(nullptr, ",")) {
          const char* dash = strchr(t, '-');
          if (dash && dash != t) {
            const int a = atoi(t), b = atoi(dash + 1);
            for (int d = a; d <= b; d++) o.devices.push_back(d);
          } else
            o.devices.push_back(getInt(t));
        }
        break;
      }
      case 'h': usage();
      default: exit(EXIT_FAILURE);
    }
  if (optind < argc) die(argv[optind], ": unknown command-line argument");
  if ((o.peaksOpt && !o.outFile && !o.eventsOnly) || (o.peaksOnly && !o.logFile) || (!o.peaksOnly && !o.inFile)) {
    fprintf(stderr, "Error! Need input/output files\n");
    usage();
  }
  // (the counts are counted in the peaks this run calls: nothing to count in with -P, -X or --events-only)
  if (o.countsFile && !o.callsPeaks()) die("", "--counts needs the peaks of this run (not with -P or -X)");
  // (the signal is taken in the peaks this run calls, from the events the library keeps: none with -X, -P or --events-only)
  if (o.peakSignalFile && !o.callsPeaks())
    die("", "--peak-signal needs the peaks and the intervals of this run (not with -X, -P or --events-only)");
  // (the summits are taken in the peaks this run calls, from the events the library keeps: none with -X, -P or --events-only)
  if (o.summitsFile && !o.callsPeaks())
    die("", "--summits needs the peaks and the intervals of this run (not with -X, -P or --events-only)");
  if ((o.summitsProminenceOpt || o.summitsHeightOpt) && !o.summitsFile) die("", "--summits-prominence and --summits-height need --summits FILE");
  if ((o.regionsBed != nullptr) != (o.regionCountsFile != nullptr)) die("", "--count-regions BED and --region-counts FILE need each other");
  // (the regions count the events the library keeps: none with -P or --events-only; -X is fine)
  if (o.regionsBed && !o.buildsPileups()) die("", "--count-regions needs the intervals of this run (not with -P or --events-only)");
  // (the tracks are made of the pileups this run builds: none with -P or --events-only; -X is fine)
  if (o.coveragePrefix && !o.buildsPileups()) die("", "--coverage needs the pileups of this run (not with -P or --events-only)");
  // (the matrix is made of the same bins: one bin size per run)
  if (o.correlationFile && !o.buildsPileups()) die("", "--correlation needs the pileups of this run (not with -P or --events-only)");
  if (o.spearmanFile && !o.buildsPileups()) die("", "--spearman needs the pileups of this run (not with -P or --events-only)");
  if (o.corrSkipZeros && !o.correlationFile && !o.spearmanFile) die("", "--corr-skip-zeros needs --correlation FILE or --spearman FILE");
  if (o.fingerprintFile && !o.buildsPileups()) die("", "--fingerprint needs the pileups of this run (not with -P or --events-only)");
  if (o.fingerprintMetricsFile && !o.fingerprintFile) die("", "--fingerprint-metrics needs --fingerprint FILE");
  // (the complexity counts the events the library keeps: none with -P or --events-only; -X is fine)
  if (o.complexityFile && !o.buildsPileups()) die("", "--complexity needs the intervals of this run (not with -P or --events-only)");
  if (o.complexityHistFile && !o.complexityFile) die("", "--complexity-hist needs --complexity FILE");
  // (the lengths and tallies count the events the library keeps: none with -P or --events-only; -X is fine)
  if ((o.lengthsFile || o.lengthsMetricsFile || o.chromStatsFile) && !o.buildsPileups())
    die("", "--lengths, --lengths-metrics and --chrom-stats need the intervals of this run (not with -P or --events-only)");
  if (o.lengthsCutsOpt && !o.lengthsMetricsFile) die("", "--lengths-cuts needs --lengths-metrics FILE");
  // (the tags are taken where this run's alignments become intervals: none with -P or --events-only; -X is fine)
  if (o.xcorOn() && !o.buildsPileups()) die("", "--xcor and --xcor-metrics need the alignments of this run (not with -P or --events-only)");
  if ((o.xcorShiftsOpt || o.xcorReadLen || o.xcorUnpaired) && !o.xcorOn())
    die("", "--xcor-shifts, --xcor-read-length and --xcor-unpaired need --xcor FILE or --xcor-metrics FILE");
  // (the distribution is taken from the pileups this run builds: none with -P or --events-only; -X is fine)
  if ((o.depthFile || o.depthMetricsFile) && !o.buildsPileups())
    die("", "--depth and --depth-metrics need the pileups of this run (not with -P or --events-only)");
  // (the curve is made of this run's peaks and of the events the library keeps: none with -X, -P or --events-only)
  if (o.saturationFile && !o.callsPeaks())
    die("", "--saturation needs the peaks and the intervals of this run (not with -X, -P or --events-only)");
  if ((o.saturationStepsOpt || o.saturationSeedOpt || o.saturationControls) && !o.saturationFile)
    die("", "--saturation-steps, --saturation-seed and --saturation-controls need --saturation FILE");
  if (o.saturationFile && (o.saturationSteps < 1 || o.saturationSteps > 100)) die("", "--saturation-steps must be in [1, 100]");
  // (the re-call on several contexts needs the collectives between their child contexts)
  if (o.saturationFile && o.devices.size() > 1) die("", "--saturation takes one device (not with --devices of more than one)");
  // (the calls are made of this run's peaks and of the events the library keeps: none with -X, -P or --events-only)
  if (o.reproOn() && !o.callsPeaks())
    die("", "--reproducibility needs the peaks and the intervals of this run (not with -X, -P or --events-only)");
  if ((o.reproPctOpt || o.reproSeedOpt || o.reproPrefix) && !o.reproOn())
    die("", "--reproducibility-overlap, --reproducibility-seed and --reproducibility-peaks need --reproducibility FILE or --reproducibility-metrics FILE");
  if (o.reproOn() && o.devices.size() > 1) die("", "--reproducibility takes one device (not with --devices of more than one)");
  if (o.gcBiasFile && !o.genomeFile) die("", "--gc-bias needs the reference sequence (--genome FASTA)");
  if (o.gcPeaksFile && !o.genomeFile) die("", "--gc-peaks needs the reference sequence (--genome FASTA)");
  if (o.gcWindowOpt && !o.gcBiasFile) die("", "--gc-window needs --gc-bias FILE");
  if (o.motifsFile && !o.genomeFile) die("", "--motifs needs the reference sequence (--genome FASTA)");
  if (o.motifsFile && !o.motifHitsFile && !o.motifSummaryFile) die("", "--motifs needs --motif-hits FILE or --motif-summary FILE");
  if ((o.motifHitsFile || o.motifSummaryFile || o.motifPvalueOpt || o.motifPseudoOpt) && !o.motifsFile)
    die("", "--motif-hits, --motif-summary, --motif-pvalue and --motif-pseudocount need --motifs FILE");
  // (the motifs are scanned in the peaks this run calls, on a device context: -P has neither)
  if (o.motifsFile && !o.callsPeaks()) die("", "--motifs needs the peaks of this run on a device (not with -X, -P or --events-only)");
  if (o.genomeFile && !o.gcBiasFile && !o.gcPeaksFile && !o.motifsFile) die("", "--genome needs --gc-bias FILE or --gc-peaks FILE");
  // (the bias counts the events the library keeps: none with -P or --events-only; -X is fine)
  if (o.gcBiasFile && !o.buildsPileups()) die("", "--gc-bias needs the intervals of this run (not with -P or --events-only)");
  // (the content is taken in the peaks this run calls, on a device context: -P has neither)
  if (o.gcPeaksFile && !o.callsPeaks()) die("", "--gc-peaks needs the peaks of this run on a device (not with -X, -P or --events-only)");
  // the treatment / control lists, and the samples they name: one per -t file and per -c file that is not "null", known before
  // anything is read or written
  const std::vector<std::string> tFiles = splitList(o.inFile), cFiles = splitList(o.ctrlFile);
  std::vector<const char*> sampleNames;
  for (size_t r = 0; r < tFiles.size(); r++) {
    sampleNames.push_back(tFiles[r].c_str());
    if (r < cFiles.size() && cFiles[r] != "null") sampleNames.push_back(cFiles[r].c_str());
  }
  if (sampleNames.size() > 32) {
    if (o.correlationFile) die("", "--correlation takes at most 32 samples");
    if (o.spearmanFile) die("", "--spearman takes at most 32 samples");
    if (o.fingerprintFile) die("", "--fingerprint takes at most 32 samples");
  }
  if ((o.coverageScaleOpt && !o.coveragePrefix) || (o.binSizeOpt && !o.coveragePrefix && !o.correlationFile && !o.fingerprintFile && !o.spearmanFile))
    die("", "--bin-size and --coverage-scale need --coverage PREFIX");
  if ((o.coveragePrefix || o.correlationFile || o.fingerprintFile || o.spearmanFile) && (o.binSize < 1 || o.binSize > (1 << 20))) die("", "--bin-size must be in [1, 1048576]");
  if ((o.profileBed != nullptr) != (o.profilePrefix != nullptr)) die("", "--profile BED and --profile-out PREFIX need each other");
  if ((o.flankOpt || o.profileBinOpt || o.profileAtOpt || o.profileMatrix) && !o.profileBed)
    die("", "--flank, --profile-bin, --profile-at and --profile-matrix need --profile BED");
  // (the profiles are made of the pileups this run builds: none with -P or --events-only; -X is fine)
  if (o.profileBed && !o.buildsPileups()) die("", "--profile needs the pileups of this run (not with -P or --events-only)");
  if (o.profileBed) {   // (the library's limits: gx_set_profile)
    if (o.profileBin < 1) die("", "--profile: --profile-bin must be at least 1");
    if (o.flank < 1 || o.flank > (1 << 20)) die("", "--profile: --flank must be in [1, 1048576]");
    if (o.flank % o.profileBin) die("", "--profile: --flank must be a multiple of --profile-bin");
    if (2 * o.flank / o.profileBin > 1024) die("", "--profile: at most 1024 bins (2 * flank / profile-bin)");
  }
  if (o.avgExtOpt) { o.singleOpt = true; o.extendOpt = false; }
  if (o.extendOpt) {
    o.singleOpt = true;
    if (o.extend <= 0) die("", "Extension length must be > 0");
  }
  if (o.atacOpt) {
    o.avgExtOpt = o.extendOpt = false;
    if (o.atacLen5 <= 0) die("", "ATAC-seq interval length must be > 0");
    o.atacLen3 = (int)(o.atacLen5 / 2.0f + 0.5f);
    o.atacLen5 /= 2;
  }
  if (o.minLen < 0) die("", "Minimum peak length must be >= 0");
  if (o.minAUC < 0.0f) die("", "Minimum AUC must be >= 0.0");
  if (o.asDiff < 0.0f) die("", "Secondary alignment score threshold must be >= 0.0");
  S.xchr = splitList(o.xchrom);
  S.threads = splitThreads(nThreads);
  if (o.pqvalue <= 0.0f || o.pqvalue > 1.0f) die("", "p-/q-value must be in (0,1]");
  const float thr = -log10f(o.pqvalue);

  if (o.xFile) loadBED(S, o.xFile);
  if (o.regionsBed) loadRegionRows(S, o.regionsBed, S.regions, nullptr);
  if (o.profileBed && !o.peaksOnly) {
    loadRegionRows(S, o.profileBed, S.anchorRows, &S.anchorStrand);
    if (S.anchorRows.empty()) die(o.profileBed, ": --profile: no anchors");
    if (o.profileMatrix && S.anchorRows.size() * (size_t)(2 * o.flank / o.profileBin) > ((size_t)1 << 26))
      die("", "--profile-matrix: more than 2^26 cells (BED lines times bins)");
  }
  if (o.peaksOnly) {  // runProgram 5398-5403
    peaksOnly(S, thr);
    return EXIT_SUCCESS;
  }
  if (o.bedFile) { S.bed = openWrite(o.bedFile, o.gzOut); S.bedOpt = true; }
  if (o.dupsOpt && o.dupsFile) { S.dups = openWrite(o.dupsFile, o.gzOut); S.dupsVerb = true; }  // 5411-5415
  // (--events-only writes nothing but the -b file: without one there is nothing the checks could change)
  if (o.eventsOnly) S.hot.on = o.bedFile != nullptr && getenv("GENRICH_NO_INT16") == nullptr;
  if (!o.eventsOnly) {
    gx_params par{};
    par.thr = thr;
    par.qval_opt = o.qvalOpt;
    par.min_auc = o.minAUC;
    par.min_len = o.minLen;
    par.max_gap = o.maxGap;
    par.device = o.device;
    par.genome_len = o.genomeLen;
    if (o.devices.empty()) o.devices.push_back(o.device);
    if (o.devices.size() > 64) die("", "at most 64 devices");
    Devs& D = S.devs;
    for (int d : o.devices) {
      par.device = d;
      gx_ctx* g = nullptr;
      int rc = gx_create(&g, &par);
      if (rc) die(g ? gx_last_error(g) : gx_strerror(rc), "");
      check(S, gx_set_keep_pileups(g, o.logFile || o.pileFile), g);  // only -f / -k print pileup values
      if (o.asDiff > 0.0f) check(S, gx_expect_fractional(g, 1), g);  // (-s: multimapping reads get weights 1/k)
      if (o.countsFile || o.peakSignalFile || o.summitsFile || o.regionsBed || o.complexityFile || o.saturationFile || o.reproOn() || o.lengthsFile || o.lengthsMetricsFile || o.chromStatsFile || o.gcBiasFile)
        check(S, gx_set_count_in_peaks(g, 1), g);
      D.ctx.push_back(g);
    }
    S.gx = D.ctx[0];
    S.hot.on = getenv("GENRICH_NO_INT16") == nullptr;  // (saveInterval's int16 checks, read by read: HotWindows)
    D.buf.resize(D.n());
    D.tagBuf.resize(D.n());
    if (D.n() > 1) {
      const int W = (int)D.n();
      bool distinct = true;
      for (int a = 0; a < W; a++)
        for (int b = a + 1; b < W; b++) distinct = distinct && o.devices[a] != o.devices[b];
      if (distinct) {
        // the library's own collectives: one RCCL communicator over the devices (xGMI), joined side by side
        char id[128];
        int rc = gx_rccl_unique_id(id, sizeof id);
        if (rc) die(gx_strerror(rc), "");
        onEachDevice(S, [&](int g) { return gx_set_rccl(D.ctx[g], g, W, id); });
      } else {
        // a device named twice (RCCL wants one rank per GPU): the exchanges go through host callbacks between
        // the threads -- the library's validation mode, here for tests on a single GPU
        pthread_barrier_init(&D.bar, nullptr, (unsigned)W);
        D.barInit = true;
        D.red.resize(W);
        D.users.resize(W);
        for (int g = 0; g < W; g++) {
          D.users[g] = Devs::User{&D, g};
          check(S, gx_set_collectives(D.ctx[g], g, W, devsAllreduce, &D.users[g]), D.ctx[g]);
        }
      }
    }
  }

  // loop over the comma-separated treatment / control lists (runProgram 5455-5585)
  for (size_t r = 0; r < tFiles.size(); r++) {  // pre-scan of every header, reference order
    scanHeader(S, tFiles[r].c_str(), false);
    if (r < cFiles.size() && cFiles[r] != "null") scanHeader(S, cFiles[r].c_str(), true);
  }
  sendChroms(S);
  if (o.coveragePrefix || o.correlationFile || o.fingerprintFile || o.spearmanFile)
    for (gx_ctx* g : S.devs.ctx) check(S, gx_set_coverage_bins(g, (uint32_t)o.binSize), g);
  if (o.depthFile || o.depthMetricsFile)
    for (gx_ctx* g : S.devs.ctx) check(S, gx_set_depth_hist(g, 1), g);
  if (o.xcorOn())
    for (gx_ctx* g : S.devs.ctx) check(S, gx_set_xcor(g, o.xcorLo, o.xcorHi), g);
  if (o.motifsFile) loadMotifs(S);
  if (o.genomeFile) loadGenome(S);
  ProfilePlan profilePlan;
  if (o.profileBed) {
    profilePlan = planProfile(S);
    for (gx_ctx* g : S.devs.ctx)
      check(S, gx_set_profile(g, profilePlan.anchors.data(), profilePlan.anchors.size(), (uint32_t)o.flank, (uint32_t)o.profileBin,
                              o.profileMatrix), g);
  }
  for (size_t r = 0; r < tFiles.size(); r++) {
    for (auto& ch : S.chrom) ch.save = false;
    const char* ctrlName = r < cFiles.size() ? cFiles[r].c_str() : nullptr;   // (no -c: no items)
    for (int i = 0; i < 2; i++) {
      const char* filename = i ? ctrlName : tFiles[r].c_str();
      if (i && filename && !strcmp(filename, "null")) filename = nullptr;
      if (i && !filename) {
        if (o.verbose) fprintf(stderr, "- control file #%d not provided -\n", S.sample);
        float lambda = 0;
        for (gx_ctx* g : S.devs.ctx) check(S, gx_sample_no_control(g, &lambda), g);  // (lambda is genome-wide: the same everywhere)
        if (o.verbose && S.gx) fprintf(stderr, "  Background pileup value: %f\n", lambda);
        break;
      }
      S.ctrl = i;
      S.sampleOpen = false;
      S.errCount = 0;
      S.buf.clear();
      S.tags.clear();
      In file;
      const bool isStdin = !strcmp(filename, "-");
      In& in = isStdin ? openStdin(S) : file;
      if (!isStdin) openRead(in, filename, S.threads.sam.inflate);
      // BAM or SAM?  (checkBAM 5107: the decompressed stream starts with "BAM\1")
      char magic[4] = {0};
      int got = 0;
      const bool bam = sniffBam(in, magic, got);
      if (o.verbose) fprintf(stderr, "Processing %s: %s\n", sampleLabel(S.sample, i).c_str(), filename);
      if (S.dupsVerb) fprintf(S.dups.f, "# %s: %s\n", sampleLabel(S.sample, i).c_str(), filename);
      Counts C;
      if (bam) {
        in.growWorkers(S.threads.bam.inflate);  // (the stream was opened with the SAM split's inflaters)
        readBAM(S, in, C, S.threads.bam);
      } else {
        in.unread(magic, (size_t)std::max(0, got));  // the sniffed bytes are the beginning of the first line
        readSAM(S, in, C, S.threads.sam);
      }
      checkIn(in);
      if (!isStdin) in.close();
      openSample(S);  // a file without a single usable record still opens (and closes) its sample
      if (S.gx) flushEvents(S);
      S.buf.clear();
      if (S.gx) flushTags(S);
      if (o.verbose) logCounts(S, C, bam);
      if (S.gx) {
        double fragLen = 0;
        float lambda = 0, factor = 0;
        onEachDevice(S, [&](int g) {
          double fl = 0;
          float la = 0, fa = 0;
          const int rc = gx_sample_end(S.devs.ctx[g], &fl, &la, &fa);
          if (g == 0) { fragLen = fl; lambda = la; factor = fa; }  // (genome-wide scalars: the same on every device)
          return rc;
        });
        long long dropped = 0;
        for (gx_ctx* g : S.devs.ctx) {
          long long d = 0;
          check(S, gx_saturation_dropped(g, &d), g);
          dropped += d;
        }
        if (dropped)  // saveInterval 2558-2573 warns read by read (with -v) and leaves them out of -b and of the -x average
          fprintf(stderr, "Warning! %lld alignments skipped due to overflow / underflow of the reference's 16-bit counters "
                          "(left out of the pileup as in Genrich; their -b lines and lengths were written before)\n", dropped);
        if (i && o.verbose) {
          fprintf(stderr, "  Background pileup value: %f\n", lambda);
          fprintf(stderr, "  Scaling factor for control pileup: %f\n", factor);
          if (factor > 5.0f) fprintf(stderr, "  ** Warning! Large scaling may mask true signal **\n");
        }
      }
    }
    if (S.gx) onEachDevice(S, [&](int g) { return gx_pvalues(S.devs.ctx[g]); });
    S.sample++;
  }
  if (S.bedOpt) closeOut(S.bed);
  if (S.dupsVerb) closeOut(S.dups);
  if (getenv("GENRICH_HOST_PROF")) { struct timespec ts; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); fprintf(stderr, "main thread cpu %.3f s\n", ts.tv_sec + ts.tv_nsec * 1e-9); }
  if (o.eventsOnly) return EXIT_SUCCESS;

  size_t nPeaks = 0;
  uint64_t genomeLen = 0, peakBP = 0;
  {
    std::vector<size_t> np(S.devs.n(), 0);
    std::vector<uint64_t> bp(S.devs.n(), 0);
    onEachDevice(S, [&](int g) { return gx_find_peaks(S.devs.ctx[g], &np[g], g == 0 ? &genomeLen : nullptr, &bp[g]); });
    for (size_t g = 0; g < S.devs.n(); g++) { nPeaks += np[g]; peakBP += bp[g]; }
  }
  if (o.verbose) {  // findPeaks 1103-1117, 1130-1132
    if (o.peaksOpt) {
      fprintf(stderr, "Peak-calling parameters:\n");
      fprintf(stderr, "  Genome length: %ldbp\n", (long)genomeLen);
      fprintf(stderr, "  Significance threshold: -log(%c) > %.3f\n", o.qvalOpt ? 'q' : 'p', thr);
      fprintf(stderr, "  Min. AUC: %.3f\n", o.minAUC);
      if (o.minLen) fprintf(stderr, "  Min. peak length: %dbp\n", o.minLen);
      fprintf(stderr, "  Max. gap between sites: %dbp\n", o.maxGap);
    } else {
      fprintf(stderr, "- peak-calling skipped -\n");
      fprintf(stderr, "  Genome length: %ldbp\n", (long)genomeLen);
    }
  }
  std::vector<const char*> names;
  for (auto& ch : S.chrom) names.push_back(ch.name.c_str());
  const int nChrom = (int)names.size();
  writeFile(S, o.pileFile, [&](FILE* f) {
    int rc = GX_OK;
    for (int r = 0; r < S.sample && rc == GX_OK; r++) {
      const char* cn = (size_t)r < cFiles.size() ? cFiles[r].c_str() : nullptr;
      rc = gx_write_pile_group(S.devs.ctx.data(), S.devs.owner.data(), r, names.data(), nChrom, tFiles[r].c_str(), cn, f);
    }
    return rc;
  });
  if (o.peaksOpt) {
    writeFile(S, o.outFile, [&](FILE* f) { return gx_write_narrowpeak_group(S.devs.ctx.data(), (int)S.devs.n(), names.data(), f); });
    if (o.verbose) fprintf(stderr, "Peaks identified: %d (%ldbp)\n", (int)nPeaks, (long)peakBP);
  }
  if (o.countsFile) writeCounts(S, names, sampleNames);
  if (o.peakSignalFile) writePeakSignal(S, names, (int)sampleNames.size());
  if (o.summitsFile) writeSummits(S, names);
  if (o.regionsBed) writeRegionCounts(S, sampleNames);
  if (o.coveragePrefix) writeCoverage(S, names);
  if (o.correlationFile) writeCorrelation(S);
  if (o.spearmanFile) writeSpearman(S);
  if (o.fingerprintFile) writeFingerprint(S);
  if (o.complexityFile) writeComplexity(S);
  if (o.lengthsFile || o.lengthsMetricsFile || o.chromStatsFile) writeIntervalStats(S, names);
  if (o.depthFile || o.depthMetricsFile) writeDepth(S);
  if (o.xcorOn()) writeXcor(S);
  if (o.gcBiasFile) writeGcBias(S);
  if (o.gcPeaksFile) writeGcPeaks(S, names);
  if (o.motifsFile) writeMotifs(S, names);
  if (o.saturationFile) writeSaturation(S);
  if (o.reproOn()) writeReproducibility(S, names);
  if (o.profileBed) writeProfile(S, profilePlan, sampleNames);
  writeFile(S, o.logFile, [&](FILE* f) {
    return gx_write_log_group(S.devs.ctx.data(), S.devs.owner.data(), S.sample, names.data(), nChrom, o.qvalOpt, o.peaksOpt, thr, f);
  });
  for (gx_ctx* g : S.devs.ctx) gx_destroy(g);
  return EXIT_SUCCESS;
}
