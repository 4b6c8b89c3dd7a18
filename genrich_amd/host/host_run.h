// host_run.h -- the run by stage, each a function over the State, in the order main calls them.  (a part of genrich_amd.cpp's translation unit)
#pragma once
namespace {

// the treatment / control lists, and the samples they name: one per -t file and per -c file that is not "null"
void planSamples(State& S) {
  S.tFiles = splitList(S.o.inFile);
  S.cFiles = splitList(S.o.ctrlFile);
  for (size_t r = 0; r < S.tFiles.size(); r++) {
    S.sampleNames.push_back(S.tFiles[r].c_str());
    if (S.controlOf(r)) S.sampleNames.push_back(S.controlOf(r));
  }
}

// What is refused before anything is read or written, sentence by sentence: their order decides which one an argv that breaks two
// rules gets.  In between, the options that switch others on or off (-x, -w, -j), the -e list and the thread budget.
void validate(State& S) {
  Opts& o = S.o;
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
  if (o.lengthsOn() && !o.buildsPileups())
    die("", "--lengths, --lengths-metrics and --chrom-stats need the intervals of this run (not with -P or --events-only)");
  if (o.lengthsCutsOpt && !o.lengthsMetricsFile) die("", "--lengths-cuts needs --lengths-metrics FILE");
  // (the tags are taken where this run's alignments become intervals: none with -P or --events-only; -X is fine)
  if (o.xcorOn() && !o.buildsPileups()) die("", "--xcor and --xcor-metrics need the alignments of this run (not with -P or --events-only)");
  if ((o.xcorShiftsOpt || o.xcorReadLen || o.xcorUnpaired) && !o.xcorOn())
    die("", "--xcor-shifts, --xcor-read-length and --xcor-unpaired need --xcor FILE or --xcor-metrics FILE");
  // (the distribution is taken from the pileups this run builds: none with -P or --events-only; -X is fine)
  if (o.depthOn() && !o.buildsPileups()) die("", "--depth and --depth-metrics need the pileups of this run (not with -P or --events-only)");
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
  if (o.kmersFile && !o.genomeFile) die("", "--kmers needs the reference sequence (--genome FASTA)");
  if ((o.kmerKOpt || o.kmerFlankOpt || o.kmerTopOpt) && !o.kmersFile) die("", "--kmer-k, --kmer-flank and --kmer-top need --kmers FILE");
  // (the k-mers are counted in the peaks this run calls, on a device context: -P has neither)
  if (o.kmersFile && !o.callsPeaks()) die("", "--kmers needs the peaks of this run on a device (not with -X, -P or --events-only)");
  if (o.genomeFile && !o.gcBiasFile && !o.gcPeaksFile && !o.motifsFile && !o.kmersFile) die("", "--genome needs --gc-bias FILE or --gc-peaks FILE");
  // (the bias counts the events the library keeps: none with -P or --events-only; -X is fine)
  if (o.gcBiasFile && !o.buildsPileups()) die("", "--gc-bias needs the intervals of this run (not with -P or --events-only)");
  // (the content is taken in the peaks this run calls, on a device context: -P has neither)
  if (o.gcPeaksFile && !o.callsPeaks()) die("", "--gc-peaks needs the peaks of this run on a device (not with -X, -P or --events-only)");
  if (S.sampleNames.size() > 32) {
    if (o.correlationFile) die("", "--correlation takes at most 32 samples");
    if (o.spearmanFile) die("", "--spearman takes at most 32 samples");
    if (o.fingerprintFile) die("", "--fingerprint takes at most 32 samples");
  }
  if ((o.coverageScaleOpt && !o.coveragePrefix) || (o.binSizeOpt && !o.binsOn())) die("", "--bin-size and --coverage-scale need --coverage PREFIX");
  if (o.binsOn() && (o.binSize < 1 || o.binSize > (1 << 20))) die("", "--bin-size must be in [1, 1048576]");
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
  S.threads = splitThreads(o.threads);
  if (o.pqvalue <= 0.0f || o.pqvalue > 1.0f) die("", "p-/q-value must be in (0,1]");
  S.thr = -log10f(o.pqvalue);
}

// -E, --count-regions' BED and --profile's anchors (not with -P: nothing is piled up there), with the two refusals of the anchors
void loadRegionInputs(State& S) {
  const Opts& o = S.o;
  if (o.xFile) loadBED(S, o.xFile);
  if (o.regionsBed) loadRegionRows(S, o.regionsBed, S.regions, nullptr);
  if (o.profileBed && !o.peaksOnly) {
    loadRegionRows(S, o.profileBed, S.anchorRows, &S.anchorStrand);
    if (S.anchorRows.empty()) die(o.profileBed, ": --profile: no anchors");
    if (o.profileMatrix && S.anchorRows.size() * (size_t)(2 * o.flank / o.profileBin) > ((size_t)1 << 26))
      die("", "--profile-matrix: more than 2^26 cells (BED lines times bins)");
  }
}

// -b and -R's files; with --events-only, whether saveInterval's int16 checks run
void openStreams(State& S) {
  const Opts& o = S.o;
  if (o.bedFile) { S.bed = openWrite(o.bedFile, o.gzOut); S.bedOpt = true; }
  if (o.dupsOpt && o.dupsFile) { S.dups = openWrite(o.dupsFile, o.gzOut); S.dupsVerb = true; }  // 5411-5415
  // (--events-only writes nothing but the -b file: without one there is nothing the checks could change)
  if (o.eventsOnly) S.hot.on = o.bedFile != nullptr && getenv("GENRICH_NO_INT16") == nullptr;
}
void closeStreams(State& S) {
  if (S.bedOpt) closeOut(S.bed);
  if (S.dupsVerb) closeOut(S.dups);
  if (getenv("GENRICH_HOST_PROF")) { struct timespec ts; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); fprintf(stderr, "main thread cpu %.3f s\n", ts.tv_sec + ts.tv_nsec * 1e-9); }
}

// one library context per device, with what it has to know before the chromosome table
void createContexts(State& S) {
  Opts& o = S.o;
  gx_params par{};
  par.thr = S.thr;
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
    if (keepsIntervals(o)) check(S, gx_set_count_in_peaks(g, 1), g);
    D.ctx.push_back(g);
  }
  S.gx = D.ctx[0];
  S.hot.on = getenv("GENRICH_NO_INT16") == nullptr;  // (saveInterval's int16 checks, read by read: HotWindows)
  D.buf.resize(D.n());
  D.tagBuf.resize(D.n());
}

// several contexts: what their collectives go through
void joinDevices(State& S) {
  Devs& D = S.devs;
  if (D.n() < 2) return;
  const int W = (int)D.n();
  bool distinct = true;
  for (int a = 0; a < W; a++)
    for (int b = a + 1; b < W; b++) distinct = distinct && S.o.devices[a] != S.o.devices[b];
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

// pre-scan of every header, reference order (runProgram 5455-5585); then the chromosome table is final and goes to the devices
void scanHeaders(State& S) {
  for (size_t r = 0; r < S.tFiles.size(); r++) {
    scanHeader(S, S.tFiles[r].c_str(), false);
    if (S.controlOf(r)) scanHeader(S, S.controlOf(r), true);
  }
  sendChroms(S);
  for (auto& ch : S.chrom) S.names.push_back(ch.name.c_str());
}

// What the figures need switched on in the library before the first sample: a figure whose library side needs a setter gets its
// line here.  (Not hooks of FIGURES: loadMotifs and loadGenome print and can refuse, so the order stands here.)
void enablePasses(State& S) {
  const Opts& o = S.o;
  if (o.binsOn())
    for (gx_ctx* g : S.devs.ctx) check(S, gx_set_coverage_bins(g, (uint32_t)o.binSize), g);
  if (o.depthOn())
    for (gx_ctx* g : S.devs.ctx) check(S, gx_set_depth_hist(g, 1), g);
  if (o.xcorOn())
    for (gx_ctx* g : S.devs.ctx) check(S, gx_set_xcor(g, o.xcorLo, o.xcorHi), g);
  if (o.motifsFile) loadMotifs(S);
  if (o.genomeFile) loadGenome(S);
  if (o.profileBed) {
    S.profilePlan = planProfile(S);
    for (gx_ctx* g : S.devs.ctx)
      check(S, gx_set_profile(g, S.profilePlan.anchors.data(), S.profilePlan.anchors.size(), (uint32_t)o.flank, (uint32_t)o.profileBin,
                              o.profileMatrix), g);
  }
}

// one alignment file, SAM or BAM, into the sample it opens: its events and tags to the devices, its -v counts
void readSampleFile(State& S, const char* filename, bool isCtrl) {
  const Opts& o = S.o;
  S.ctrl = isCtrl;
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
  if (o.verbose) fprintf(stderr, "Processing %s: %s\n", sampleLabel(S.sample, isCtrl).c_str(), filename);
  if (S.dupsVerb) fprintf(S.dups.f, "# %s: %s\n", sampleLabel(S.sample, isCtrl).c_str(), filename);
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
}

// the sample just read becomes a pileup on every device
void closeSample(State& S, bool isCtrl) {
  if (!S.gx) return;
  float lambda = 0, factor = 0;
  onEachDevice(S, [&](int g) {
    double fl = 0;
    float la = 0, fa = 0;
    const int rc = gx_sample_end(S.devs.ctx[g], &fl, &la, &fa);
    if (g == 0) { lambda = la; factor = fa; }  // (genome-wide scalars: the same on every device)
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
  if (isCtrl && S.o.verbose) {
    fprintf(stderr, "  Background pileup value: %f\n", lambda);
    fprintf(stderr, "  Scaling factor for control pileup: %f\n", factor);
    if (factor > 5.0f) fprintf(stderr, "  ** Warning! Large scaling may mask true signal **\n");
  }
}

// a replicate without a control file (none named, or "null")
void noControl(State& S) {
  if (S.o.verbose) fprintf(stderr, "- control file #%d not provided -\n", S.sample);
  float lambda = 0;
  for (gx_ctx* g : S.devs.ctx) check(S, gx_sample_no_control(g, &lambda), g);  // (lambda is genome-wide: the same everywhere)
  if (S.o.verbose && S.gx) fprintf(stderr, "  Background pileup value: %f\n", lambda);
}

void callPeaks(State& S) {
  const Opts& o = S.o;
  uint64_t genomeLen = 0;
  std::vector<size_t> np(S.devs.n(), 0);
  std::vector<uint64_t> bp(S.devs.n(), 0);
  onEachDevice(S, [&](int g) { return gx_find_peaks(S.devs.ctx[g], &np[g], g == 0 ? &genomeLen : nullptr, &bp[g]); });
  for (size_t g = 0; g < S.devs.n(); g++) { S.nPeaks += np[g]; S.peakBP += bp[g]; }
  if (!o.verbose) return;  // findPeaks 1103-1117, 1130-1132
  if (o.peaksOpt) logPeakParams(o, genomeLen, S.thr);
  else fprintf(stderr, "- peak-calling skipped -\n  Genome length: %ldbp\n", (long)genomeLen);
}

// -k, -o, every figure that is on in FIGURES' order, -f
void writeOutputs(State& S) {
  const Opts& o = S.o;
  const int nChrom = (int)S.names.size();
  writeFile(S, o.pileFile, [&](FILE* f) {
    int rc = GX_OK;
    for (int r = 0; r < S.sample && rc == GX_OK; r++) {
      const char* cn = (size_t)r < S.cFiles.size() ? S.cFiles[r].c_str() : nullptr;
      rc = gx_write_pile_group(S.devs.ctx.data(), S.devs.owner.data(), r, S.names.data(), nChrom, S.tFiles[r].c_str(), cn, f);
    }
    return rc;
  });
  if (o.peaksOpt) {
    writeFile(S, o.outFile, [&](FILE* f) { return gx_write_narrowpeak_group(S.devs.ctx.data(), (int)S.devs.n(), S.names.data(), f); });
    if (o.verbose) fprintf(stderr, "Peaks identified: %d (%ldbp)\n", (int)S.nPeaks, (long)S.peakBP);
  }
  for (const Figure& fig : FIGURES)
    if (fig.on(o)) fig.write(S);
  writeFile(S, o.logFile, [&](FILE* f) {
    return gx_write_log_group(S.devs.ctx.data(), S.devs.owner.data(), S.sample, S.names.data(), nChrom, o.qvalOpt, o.peaksOpt, S.thr, f);
  });
}

}  // namespace
