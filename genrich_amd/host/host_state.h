// host_state.h -- the run's state: options, the thread budget, the chromosome table with its -e / -E, the device contexts and what
// is sent to all of them, HotWindows (saveInterval's int16 checks).  (a part of genrich_amd.cpp's translation unit)
#pragma once
namespace {

// ---- chromosome table (saveChrom 4220-4270, saveXBed 1144-1206) -----------------------------
struct Chrom {
  std::string name;
  uint32_t len = 0;
  bool skip = false, save = false;
  std::vector<uint32_t> bed;  // merged start/end pairs
};
struct BedRec { std::string name; uint32_t pos[2]; };

struct Opts {
  const char *inFile = nullptr, *ctrlFile = nullptr, *outFile = nullptr, *logFile = nullptr, *pileFile = nullptr,
             *bedFile = nullptr, *xFile = nullptr, *dupsFile = nullptr, *xchrom = nullptr,
             *countsFile = nullptr,  // --counts: each sample's intervals counted in the peaks (no Genrich counterpart)
             *peakSignalFile = nullptr,  // --peak-signal: each sample's own depth inside the peaks: height, summit, area
             *summitsFile = nullptr,  // --summits: the local maxima of the treatments' pooled depth inside the peaks
             *regionsBed = nullptr, *regionCountsFile = nullptr,  // --count-regions BED --region-counts FILE: ... in given regions
             *coveragePrefix = nullptr,  // --coverage PREFIX: a binned bedGraph track per sample (no Genrich counterpart)
             *profileBed = nullptr, *profilePrefix = nullptr;  // --profile BED --profile-out PREFIX: signal around anchor sites
  int flank = 2000, profileBin = 10;   // --flank, --profile-bin
  bool flankOpt = false, profileBinOpt = false, profileAtOpt = false, profileCenter = false, profileMatrix = false;
  int binSize = 50;             // --bin-size
  double coverageScale = 1.0;   // --coverage-scale
  bool binSizeOpt = false, coverageScaleOpt = false;
  bool binsOn() const;                     // some figure that is made of the coverage bins is on (FIGURES, host_figures.h)
  const char* correlationFile = nullptr;   // --correlation FILE: the samples' Pearson matrix from the coverage bins
  bool corrSkipZeros = false;              // --corr-skip-zeros (both matrices)
  const char* spearmanFile = nullptr;      // --spearman FILE: the samples' Spearman matrix from the coverage bins
  const char* fingerprintFile = nullptr;   // --fingerprint FILE: each sample's Lorenz curve from the coverage bins
  const char* fingerprintMetricsFile = nullptr;   // --fingerprint-metrics FILE: ... and its figures
  const char* complexityFile = nullptr;    // --complexity FILE: each sample's library complexity from its kept intervals
  const char* depthFile = nullptr;         // --depth FILE: each sample's per-base depth distribution from its pileup
  const char* depthMetricsFile = nullptr;  // --depth-metrics FILE: ... and the figures made of it
  bool depthOn() const { return depthFile || depthMetricsFile; }
  const char* lengthsFile = nullptr;        // --lengths FILE: each sample's interval lengths from its kept intervals
  const char* lengthsMetricsFile = nullptr; // --lengths-metrics FILE: ... and the figures made of them
  const char* chromStatsFile = nullptr;     // --chrom-stats FILE: ... and its intervals per chromosome
  std::vector<uint64_t> lengthsCuts{150, 300, 500};   // --lengths-cuts A,B,...: the class borders of the metrics' shares
  bool lengthsCutsOpt = false;
  bool lengthsOn() const { return lengthsFile || lengthsMetricsFile || chromStatsFile; }
  const char* xcorFile = nullptr;           // --xcor FILE: each sample's strand cross-correlation curve from its alignments' 5' ends
  const char* xcorMetricsFile = nullptr;    // --xcor-metrics FILE: ... and the figures made of it (fragment length, NSC, RSC)
  int xcorLo = -100, xcorHi = 600;          // --xcor-shifts LO,HI
  bool xcorShiftsOpt = false;
  int xcorReadLen = 0;                      // --xcor-read-length R: the phantom peak sits at R - 1 (0: not given)
  bool xcorUnpaired = false;                // --xcor-unpaired: only unpaired alignments give tags
  bool xcorOn() const { return xcorFile || xcorMetricsFile; }
  const char* complexityHistFile = nullptr;   // --complexity-hist FILE: ... and its duplication histogram
  const char* saturationFile = nullptr;    // --saturation FILE: the peaks called once more on nested subsamples of the run's intervals
  int saturationSteps = 10;                // --saturation-steps N: the points of the curve, T_j = (j << 32) / N
  bool saturationStepsOpt = false;
  uint64_t saturationSeed = 1;             // --saturation-seed S
  bool saturationSeedOpt = false;
  bool saturationControls = false;         // --saturation-controls: the controls are subsampled too
  const char* reproFile = nullptr;         // --reproducibility FILE: the peaks called once more on every replicate, its halves and the pools of halves
  const char* reproMetricsFile = nullptr;  // --reproducibility-metrics FILE: Nt, Np, N_self, the two ratios and the verdict (it may stand alone)
  int reproPct = 50;                       // --reproducibility-overlap PCT: a peak supports another over PCT % of the shorter
  bool reproPctOpt = false;
  uint64_t reproSeed = 1;                  // --reproducibility-seed S
  bool reproSeedOpt = false;
  const char* reproPrefix = nullptr;       // --reproducibility-peaks PREFIX: every call's narrowPeak, the conservative and the optimal set
  bool reproOn() const { return reproFile || reproMetricsFile; }
  int summitsProminence = 25, summitsHeight = 50;   // --summits-prominence PCT, --summits-height PCT
  bool summitsProminenceOpt = false, summitsHeightOpt = false;
  const char* genomeFile = nullptr;        // --genome FASTA: the reference sequence, to the devices as two bit vectors
  const char* gcBiasFile = nullptr;        // --gc-bias FILE: each sample's GC bias (observed over expected windows per GC percent)
  int gcWindow = 200;                      // --gc-window W
  bool gcWindowOpt = false;
  const char* gcPeaksFile = nullptr;       // --gc-peaks FILE: the GC content of every called peak
  const char* motifsFile = nullptr;        // --motifs FILE: JASPAR count matrices, scanned in the called peaks on the device
  const char* motifHitsFile = nullptr;     // --motif-hits FILE: every hit, BED-like
  const char* motifSummaryFile = nullptr;  // --motif-summary FILE: per motif the peaks' and the genome's counts and the enrichment
  double motifPvalue = 1e-4, motifPseudo = 1.0;   // --motif-pvalue P, --motif-pseudocount X
  bool motifPvalueOpt = false, motifPseudoOpt = false;
  const char* kmersFile = nullptr;         // --kmers FILE: the k-mers of the called peaks against the whole genome
  int kmerK = 8, kmerFlank = -1, kmerTop = 100;   // --kmer-k K, --kmer-flank N (none: the whole peaks), --kmer-top N (0: all)
  bool kmerKOpt = false, kmerFlankOpt = false, kmerTopOpt = false;
  uint64_t genomeLen = 0;
  int extend = 0, minMapQ = 0, minLen = 0, maxGap = 100, atacLen5 = 100, atacLen3 = 0;
  float asDiff = 0.0f, pqvalue = 0.01f, minAUC = 200.0f;
  bool singleOpt = false, extendOpt = false, avgExtOpt = false, atacOpt = false, atacAdj = true, gzOut = false,
       qvalOpt = false, dupsOpt = false, peaksOpt = true, peaksOnly = false, sortOpt = true, verbose = false,
       eventsOnly = false;
  int device = 0;
  int threads = 1;           // --threads N, else GENRICH_THREADS, else up to 16 of the machine's cores (parseOptions)
  std::vector<int> devices;  // --devices a,b,...: one context per GPU, chromosomes sharded by length
  // what a figure is made of: the run's intervals, pileups and alignments (none with -P or --events-only) ...
  bool buildsPileups() const { return !peaksOnly && !eventsOnly; }
  bool callsPeaks() const { return buildsPileups() && peaksOpt; }   // ... and for some its peaks as well (none with -X either)
};

// --threads N sizes three pools next to the reader and the state's owner: BGZF inflaters, record decoders (1: records are decoded on
// the parsing thread) and state workers.  BAM: inflating the blocks is ~90 % of the ingest's CPU time (binary records decode in no
// time), so a BAM stream gets its own split of the budget once it has been recognised.
struct ThreadSplit { int inflate = 1, decode = 1, state = 1; };
struct Threads { ThreadSplit sam, bam; };

// ---- several GPUs of one node -------------------------------------------------------
// One library context per device, chromosomes dealt out by longest-processing-time bin packing; every event
// goes to the context that owns its chromosome; gx_sample_end / gx_pvalues / gx_find_peaks run on one host
// thread per device because they contain the run's collectives (fragLen sums, the BH table): RCCL inside the
// library when the devices are distinct, in-process callbacks when a device is named twice (a test on one GPU).
struct Devs {
  std::vector<gx_ctx*> ctx;
  std::vector<int> owner;                       // chromosome -> index into ctx
  std::vector<std::vector<gx_event>> buf;       // events on their way to each context
  std::vector<std::vector<gx_tag>> tagBuf;      // --xcor: ... and tags
  // in-process collectives (callback mode)
  pthread_barrier_t bar;
  bool barInit = false;
  std::vector<std::vector<int64_t>> red;
  struct User { Devs* d; int rank; };
  std::vector<User> users;
  size_t n() const { return ctx.size(); }
};

int devsAllreduce(int64_t* buf, size_t n, void* user) {
  Devs::User* u = static_cast<Devs::User*>(user);
  Devs& D = *u->d;
  D.red[u->rank].assign(buf, buf + n);
  pthread_barrier_wait(&D.bar);
  for (size_t k = 0; k < n; k++) {
    int64_t sum = 0;
    for (size_t r = 0; r < D.n(); r++) sum += D.red[r][k];
    buf[k] = sum;
  }
  pthread_barrier_wait(&D.bar);
  return 0;
}

// ---- saveInterval's int16 checks, read by read (Genrich.c:2558-2573) ----------------------------------------------
// The reference drops an alignment whose start lies on a base where its int16 difference already holds 32,767, or whose
// end lies on one that holds -32,768: a warning with -v, no -b line, length 0 towards the -x average.  The library
// reproduces the effect on the pileup by itself (gx_sample_end); what the reference PRINTS needs the decision when the
// read is saved, in input order.  A base can only get there when its 4096-base window holds 32,766 starts (or ends), so:
// the thread that owns the state counts the weight of starts and of ends per window (two increments per event); a window
// that comes that far is "loaded" -- its exact difference per base so far comes from the device, which has every event
// pushed up to now (gx_window_net) -- and kept on the host from then on.  Reads that touch a loaded window, or bring one
// to the threshold, are decided on exact state; everything else cannot be dropped.  Real data never loads a window.
struct HotWindows {
  static constexpr int WB = 12;
  static constexpr uint32_t WMASK = (1u << WB) - 1u;
  bool on = false;
  std::vector<size_t> base;                                   // first window of a chromosome (position `len` has an entry)
  std::vector<uint32_t> ws, we;                               // weight (1/120) of the sample's starts / ends per window
  std::unordered_map<size_t, std::vector<long long>> win;     // loaded windows: the exact difference per base
  // --events-only -b (no device to ask for a window's state): the sample's events so far, 16 bytes each -- 1.6 GB per 10^8
  // fragments, scanned once per window that comes near the limits (real data: none).  GENRICH_NO_INT16=1 drops the copy
  // (and the read-by-read decisions) for event dumps of that size.
  std::vector<gx_event> all;
  void init(const std::vector<Chrom>& chrom) {
    base.assign(chrom.size() + 1, 0);
    for (size_t c = 0; c < chrom.size(); c++) base[c + 1] = base[c] + ((size_t)chrom[c].len >> WB) + 1;
    ws.assign(base.back(), 0);
    we.assign(base.back(), 0);
    win.clear();
    all.clear();
  }
  // an event of a chunk that the workers prepared: counted; true when it has to be decided on exact state instead
  bool add(const gx_event& e) {
    const uint32_t w = (uint32_t)gxsat::weight_of(e.count);
    const size_t a = base[e.chrom] + (e.start >> WB), b = base[e.chrom] + (e.end >> WB);
    ws[a] += w;
    we[b] += w;
    return ws[a] >= (uint32_t)gxsat::HOT || we[b] >= (uint32_t)gxsat::HOT || (!win.empty() && (win.count(a) || win.count(b)));
  }
  void sub(const gx_event& e) {
    const uint32_t w = (uint32_t)gxsat::weight_of(e.count);
    ws[base[e.chrom] + (e.start >> WB)] -= w;
    we[base[e.chrom] + (e.end >> WB)] -= w;
  }
};

struct RegionRow { std::string chrom, name; uint32_t start, end; bool named; };   // a line of --count-regions' BED

// Chromosome name -> index.  A name that no header has gets an index behind the table (the library counts nothing there, its row
// is zero) and its place behind the table's names.
struct ChromNames {
  std::vector<const char*> all;   // the table's names, then the unknown ones (good while the strings given to of() live)
  std::unordered_map<std::string, uint32_t> idx;
  ChromNames() = default;
  explicit ChromNames(const std::vector<Chrom>& chrom) {
    for (const Chrom& c : chrom) {
      idx.emplace(c.name, (uint32_t)all.size());
      all.push_back(c.name.c_str());
    }
  }
  uint32_t of(const std::string& name) {
    auto it = idx.find(name);
    if (it == idx.end()) {
      it = idx.emplace(name, (uint32_t)all.size()).first;
      all.push_back(name.c_str());
    }
    return it->second;
  }
};
struct ProfilePlan {                   // --profile: what the anchors' BED becomes once the chromosome table is final (planProfile)
  ChromNames names;                    // the table's names, then those of chromosomes that no header names
  std::vector<gx_anchor> anchors;
  std::vector<gx_region> regions;
  std::vector<const char*> rowNames;
  size_t counted = 0;                  // anchors on chromosomes the run computes: known, not -e skipped, not empty
};

struct State {
  Opts o;
  Threads threads;           // (set once, after the options)
  std::vector<std::string> tFiles, cFiles;   // (what a stage leaves for those behind it, host_run.h:) the -t / -c lists ...
  std::vector<const char*> sampleNames;      // ... and the files that are read, in run order (planSamples)
  const char* controlOf(size_t r) const { return r < cFiles.size() && cFiles[r] != "null" ? cFiles[r].c_str() : nullptr; }
  float thr = 0.0f;                          // -log10 of -p / -q (validate)
  std::vector<const char*> names;            // the chromosome table's names, once it is final (scanHeaders)
  ProfilePlan profilePlan;                   // (enablePasses)
  size_t nPeaks = 0, peakBP = 0;             // (callPeaks)
  std::vector<Chrom> chrom;
  std::vector<std::string> xchr;
  std::vector<BedRec> xbed;
  std::vector<RegionRow> regions;   // --count-regions, in the BED's order
  std::vector<RegionRow> anchorRows;   // --profile, in the BED's order ...
  std::vector<int> anchorStrand;       // ... and each line's strand, +1 / -1
  gx_ctx* gx = nullptr;      // the (first) device context; nullptr with --events-only
  Devs devs;                 // all of them
  bool tableFrozen = false;  // the device already holds the chromosome table
  std::unique_ptr<gxhost::Input> stdinIn;  // '-' can be opened once: its header pre-scan is replayed to the real pass
  bool sampleOpen = false;   // gx_sample_begin done for the file being read
  std::vector<gx_event> buf;
  std::vector<gx_tag> tags;  // --xcor: the strand-tagged 5' ends on their way to the device
  bool unpairedTags = false; // ... and some of them came from unpaired alignments
  Out bed;
  bool bedOpt = false;
  Out dups;               // -R: log of the reads removed as PCR duplicates
  bool dupsVerb = false;
  bool ctrl = false;
  int sample = 0;
  uint64_t errCount = 0;
  HotWindows hot;            // (with a device: saveInterval's int16 checks)
  // --motifs: the matrices read, their scores (row j: A C G T), the records the library takes and each threshold's achieved p
  std::vector<gxhost::MotifRec> motifs;
  std::vector<int16_t> motifScores;
  std::vector<gx_motif> motifRecs;
  std::vector<double> motifP;   // (NaN: the motif cannot hit)
};

void check(State& S, int rc, gx_ctx* which = nullptr) {
  if (rc == GX_OK) return;
  gx_ctx* g = which ? which : S.gx;
  std::string detail = g ? gx_last_error(g) : "";
  die(detail.empty() ? std::string(gx_strerror(rc)) : detail, "");
}

// f(context index) on every device context: in place for one, one host thread each for several (the calls
// that contain collectives must run side by side); the first failure ends the program like any other,
template <typename F>
void onEachDevice(State& S, F f) {
  Devs& D = S.devs;
  if (D.n() == 1) {
    check(S, f(0), D.ctx[0]);
    return;
  }
  // A context that fails ends the program FROM ITS OWN THREAD: the others may already be waiting for it inside a
  // collective (ncclAllReduce / ncclAllGather, or the barrier of the callback mode), where a join would wait forever.
  std::vector<std::thread> th;
  for (size_t g = 0; g < D.n(); g++)
    th.emplace_back([&, g] {
      const int rc = f((int)g);
      if (rc != GX_OK) {
        const std::string detail = gx_last_error(D.ctx[g]);
        fprintf(stderr, "Error! %s\n", detail.empty() ? gx_strerror(rc) : detail.c_str());
        fflush(nullptr);
        _exit(EXIT_FAILURE);  // (no atexit handlers: the other threads' device work is still in flight)
      }
    });
  for (auto& t : th) t.join();
}

// the events gathered so far go to the contexts that own their chromosomes
void flushEvents(State& S) {
  Devs& D = S.devs;
  if (D.n() == 1) {
    if (!S.buf.empty()) check(S, gx_push_events(S.gx, S.buf.data(), S.buf.size()));
    return;
  }
  for (auto& b : D.buf) b.clear();
  for (const gx_event& e : S.buf) D.buf[D.owner[e.chrom]].push_back(e);
  for (size_t g = 0; g < D.n(); g++)
    if (!D.buf[g].empty()) check(S, gx_push_events(D.ctx[g], D.buf[g].data(), D.buf[g].size()), D.ctx[g]);
}

// --xcor: the tags gathered so far go to the contexts that own their chromosomes (their order does not matter)
void flushTags(State& S) {
  Devs& D = S.devs;
  if (S.tags.empty()) return;
  if (D.n() == 1) check(S, gx_push_tags(S.gx, S.tags.data(), S.tags.size()));
  else {
    for (auto& b : D.tagBuf) b.clear();
    for (const gx_tag& t : S.tags) D.tagBuf[D.owner[t.chrom]].push_back(t);
    for (size_t g = 0; g < D.n(); g++)
      if (!D.tagBuf[g].empty()) check(S, gx_push_tags(D.ctx[g], D.tagBuf[g].data(), D.tagBuf[g].size()), D.ctx[g]);
  }
  S.tags.clear();
}

void mergeBed(Chrom& c, const std::vector<BedRec>& xbed, bool verbose) {
  std::vector<std::pair<uint32_t, uint32_t>> iv;
  for (const BedRec& b : xbed)
    if (b.name == c.name) {
      if (b.pos[0] >= c.len) {
        if (verbose) {
          fprintf(stderr, "Warning! BED interval (%s, %d - %d) ignored\n", b.name.c_str(), b.pos[0], b.pos[1]);
          fprintf(stderr, "  - located off end of reference %s (length %d)\n", c.name.c_str(), c.len);
        }
        continue;
      }
      // insertion before the first interval whose start is >= this start (1165-1175)
      size_t j = 0;
      while (j < iv.size() && b.pos[0] > iv[j].first) j++;
      iv.insert(iv.begin() + j, {b.pos[0], b.pos[1]});
    }
  std::vector<std::pair<uint32_t, uint32_t>> out;
  for (auto& p : iv) {
    if (p.second > c.len) {
      if (verbose) {
        fprintf(stderr, "Warning! BED interval (%s, %d - %d) extends ", c.name.c_str(), p.first, p.second);
        fprintf(stderr, "past end of ref.\n  - edited to (%s, %d - %d)\n", c.name.c_str(), p.first, c.len);
      }
      p.second = c.len;
    }
    if (!out.empty() && p.first <= out.back().second) {
      if (p.second > out.back().second) out.back().second = p.second;
    } else
      out.push_back(p);
  }
  for (auto& p : out) {
    c.bed.push_back(p.first);
    c.bed.push_back(p.second);
  }
}

int saveChrom(State& S, const char* name, uint32_t len) {
  for (size_t i = 0; i < S.chrom.size(); i++)
    if (S.chrom[i].name == name) {
      if (S.chrom[i].len != len) die(name, ": reference sequence has different lengths in BAM/SAM files");
      if (!S.ctrl) S.chrom[i].save = true;
      return (int)i;
    }
  if (S.tableFrozen)  // every header was pre-scanned: this is an @SQ line that follows the first record of its file
    die(name, ": reference sequence first seen after the chromosome table was sent to the device");
  Chrom c;
  c.name = name;
  c.len = len;
  for (auto& x : S.xchr)
    if (x == name) c.skip = true;
  c.save = !S.ctrl;  // do not save if ref in ctrl sample only
  if (!c.skip) mergeBed(c, S.xbed, S.o.verbose);
  S.chrom.push_back(c);
  return (int)S.chrom.size() - 1;
}

void sendChroms(State& S) {
  S.tableFrozen = true;
  if (!S.gx) return;
  size_t n = S.chrom.size();
  if (!n) die("", "No analyzable genome (length=0)");
  std::vector<uint32_t> len(n);
  std::vector<uint8_t> skip(n);
  std::vector<const uint32_t*> bed(n);
  std::vector<int32_t> bedLen(n);
  for (size_t i = 0; i < n; i++) {
    len[i] = S.chrom[i].len;
    skip[i] = S.chrom[i].skip;
    bed[i] = S.chrom[i].bed.data();
    bedLen[i] = (int32_t)S.chrom[i].bed.size();
  }
  Devs& D = S.devs;
  for (gx_ctx* g : D.ctx) check(S, gx_set_chroms(g, (int)n, len.data(), skip.data(), bed.data(), bedLen.data()), g);
  D.owner.assign(n, 0);
  if (D.n() > 1) {
    // longest-processing-time bin packing of the chromosomes by length (the reference's per-chromosome loops,
    // Genrich.c:2172, 1729, 987, are independent): hg38 over 8 GPUs -> heaviest share 400 of 3088 Mbp
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return len[a] > len[b]; });
    std::vector<uint64_t> load(D.n(), 0);
    for (size_t i : order) {
      size_t best = 0;
      for (size_t g = 1; g < D.n(); g++)
        if (load[g] < load[best]) best = g;
      D.owner[i] = (int)best;
      load[best] += len[i];
    }
    for (size_t g = 0; g < D.n(); g++) {
      std::vector<uint8_t> owned(n);
      for (size_t i = 0; i < n; i++) owned[i] = D.owner[i] == (int)g;
      check(S, gx_set_owned(D.ctx[g], owned.data()), D.ctx[g]);
    }
  }
}

}  // namespace
