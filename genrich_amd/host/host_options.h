// host_options.h -- the command line: one table row per long option (its name, whether it takes an argument, what it does to Opts),
// the short options of the reference's getopt string, parseOptions.  (a part of genrich_amd.cpp's translation unit)
#pragma once
namespace {

// ---- what a row does: the makers ----------------------------------------------------------------------------------------------
typedef std::function<void(Opts&, const char*)> Action;
Action path(const char* Opts::*to) { return [=](Opts& o, const char* arg) { o.*to = arg; }; }
Action flag(bool Opts::*to) { return [=](Opts& o, const char*) { o.*to = true; }; }
Action help(void (*text)()) { return [=](Opts&, const char*) { text(); }; }
// an integer as the reference's options take it (getInt); `given` here and below: the "was given" flag of an option that has one
Action integer(int Opts::*to, bool Opts::*given = nullptr) {
  return [=](Opts& o, const char* arg) { o.*to = getInt(arg); if (given) o.*given = true; };
}
// a decimal integer in [lo, hi] and nothing else (strictInt), into an int or a uint64_t
template <class T>
Action strict(T Opts::*to, bool Opts::*given, __int128 lo, __int128 hi, const char* sentence) {
  return [=](Opts& o, const char* arg) {
    __int128 v;
    if (!strictInt(arg, lo, hi, &v)) die(arg, sentence);
    o.*to = (T)v;
    if (given) o.*given = true;
  };
}
// a double that is the whole argument and that `accepts` takes (the track's values and the motifs' scores are computed in doubles)
Action real(double Opts::*to, bool Opts::*given, bool (*accepts)(double), const char* sentence) {
  return [=](Opts& o, const char* arg) {
    char* end = nullptr;
    const double v = strtod(arg, &end);
    if (end == arg || *end != '\0' || !accepts(v)) die(arg, sentence);
    o.*to = v;
    if (given) o.*given = true;
  };
}

// ---- the irregular ones -------------------------------------------------------------------------------------------------------
void setDevices(Opts& o, const char* arg) {  // --devices 0,1,2 or 0-7
  std::string list(arg);
  for (char* t = strtok(list.data(), ","); t; t = strtok(nullptr, ",")) {
    const char* dash = strchr(t, '-');
    if (dash && dash != t) {
      const int a = atoi(t), b = atoi(dash + 1);
      for (int d = a; d <= b; d++) o.devices.push_back(d);
    } else
      o.devices.push_back(getInt(t));
  }
}
void setProfileAt(Opts& o, const char* arg) {
  if (strcmp(arg, "tss") && strcmp(arg, "center")) die(arg, ": --profile-at takes tss or center");
  o.profileCenter = !strcmp(arg, "center");
  o.profileAtOpt = true;
}
void setXcorShifts(Opts& o, const char* arg) {  // --xcor-shifts LO,HI: two integers, -4096 <= LO <= HI <= 4096
  const char* t = arg;
  __int128 lo, hi;
  if (!strictInt(t, -GX_XCOR_MAX_SHIFT, GX_XCOR_MAX_SHIFT, &lo, &t) || !t || !strictInt(t, -GX_XCOR_MAX_SHIFT, GX_XCOR_MAX_SHIFT, &hi) || lo > hi)
    die(arg, ": --xcor-shifts takes two integers LO,HI with -4096 <= LO <= HI <= 4096");
  o.xcorLo = (int)lo;
  o.xcorHi = (int)hi;
  o.xcorShiftsOpt = true;
}
void setLengthsCuts(Opts& o, const char* arg) {  // --lengths-cuts A,B,...: at most 8 ascending positive integers
  o.lengthsCuts.clear();
  o.lengthsCutsOpt = true;
  for (const char* t = arg; t;) {
    __int128 v;
    if (o.lengthsCuts.size() == GX_LEN_MAX_CUTS || !strictInt(t, 1, 0xffffffffll, &v, &t) || (!o.lengthsCuts.empty() && (uint64_t)v <= o.lengthsCuts.back()))
      die(arg, ": --lengths-cuts takes at most 8 ascending positive integers, A,B,...");
    o.lengthsCuts.push_back((uint64_t)v);
  }
}

// ---- the table ----------------------------------------------------------------------------------------------------------------
// getopt_long sees the rows in this order (it decides which abbreviations are unique); a row with `alias` is the long name of a
// short option and has no action of its own
struct LongOpt { const char* name; int arg; Action act; int alias = 0; };   // (arg: no_argument / required_argument)
const LongOpt LONG_OPTS[] = {
    {"help", no_argument, nullptr, 'h'},
    {"verbose", no_argument, nullptr, 'v'},
    {"version", no_argument, nullptr, 'V'},
    {"events-only", no_argument, flag(&Opts::eventsOnly)},
    {"device", required_argument, integer(&Opts::device)},
    {"devices", required_argument, setDevices},
    {"threads", required_argument, integer(&Opts::threads)},
    {"counts", required_argument, path(&Opts::countsFile)},
    {"peak-signal", required_argument, path(&Opts::peakSignalFile)},
    {"count-regions", required_argument, path(&Opts::regionsBed)},
    {"region-counts", required_argument, path(&Opts::regionCountsFile)},
    {"coverage", required_argument, path(&Opts::coveragePrefix)},
    {"bin-size", required_argument, integer(&Opts::binSize, &Opts::binSizeOpt)},
    {"coverage-scale", required_argument, real(&Opts::coverageScale, &Opts::coverageScaleOpt, [](double) { return true; }, ": cannot convert to float")},
    {"profile", required_argument, path(&Opts::profileBed)},
    {"profile-out", required_argument, path(&Opts::profilePrefix)},
    {"flank", required_argument, integer(&Opts::flank, &Opts::flankOpt)},
    {"profile-bin", required_argument, integer(&Opts::profileBin, &Opts::profileBinOpt)},
    {"profile-at", required_argument, setProfileAt},
    {"profile-matrix", no_argument, flag(&Opts::profileMatrix)},
    {"correlation", required_argument, path(&Opts::correlationFile)},
    {"corr-skip-zeros", no_argument, flag(&Opts::corrSkipZeros)},
    {"fingerprint", required_argument, path(&Opts::fingerprintFile)},
    {"fingerprint-metrics", required_argument, path(&Opts::fingerprintMetricsFile)},
    {"spearman", required_argument, path(&Opts::spearmanFile)},
    {"complexity", required_argument, path(&Opts::complexityFile)},
    {"complexity-hist", required_argument, path(&Opts::complexityHistFile)},
    {"saturation", required_argument, path(&Opts::saturationFile)},
    {"saturation-steps", required_argument, integer(&Opts::saturationSteps, &Opts::saturationStepsOpt)},
    {"saturation-seed", required_argument, strict(&Opts::saturationSeed, &Opts::saturationSeedOpt, 0, UINT64_MAX, ": --saturation-seed takes an integer in [0, 2^64 - 1]")},
    {"saturation-controls", no_argument, flag(&Opts::saturationControls)},
    {"depth", required_argument, path(&Opts::depthFile)},
    {"depth-metrics", required_argument, path(&Opts::depthMetricsFile)},
    {"xcor", required_argument, path(&Opts::xcorFile)},
    {"xcor-metrics", required_argument, path(&Opts::xcorMetricsFile)},
    {"xcor-shifts", required_argument, setXcorShifts},
    {"xcor-read-length", required_argument, strict(&Opts::xcorReadLen, nullptr, 1, 1000000, ": --xcor-read-length takes a positive integer (at most 1000000)")},
    {"xcor-unpaired", no_argument, flag(&Opts::xcorUnpaired)},
    {"lengths", required_argument, path(&Opts::lengthsFile)},
    {"lengths-metrics", required_argument, path(&Opts::lengthsMetricsFile)},
    {"lengths-cuts", required_argument, setLengthsCuts},
    {"chrom-stats", required_argument, path(&Opts::chromStatsFile)},
    {"reproducibility", required_argument, path(&Opts::reproFile)},
    {"reproducibility-metrics", required_argument, path(&Opts::reproMetricsFile)},
    {"reproducibility-overlap", required_argument, strict(&Opts::reproPct, &Opts::reproPctOpt, 0, 100, ": --reproducibility-overlap takes an integer in [0, 100]")},
    {"reproducibility-seed", required_argument, strict(&Opts::reproSeed, &Opts::reproSeedOpt, 0, UINT64_MAX, ": --reproducibility-seed takes an integer in [0, 2^64 - 1]")},
    {"reproducibility-peaks", required_argument, path(&Opts::reproPrefix)},
    {"help-reproducibility", no_argument, help(usageReproducibility)},
    {"summits", required_argument, path(&Opts::summitsFile)},
    {"summits-prominence", required_argument, strict(&Opts::summitsProminence, &Opts::summitsProminenceOpt, 0, 100, ": --summits-prominence takes an integer in [0, 100]")},
    {"summits-height", required_argument, strict(&Opts::summitsHeight, &Opts::summitsHeightOpt, 0, 100, ": --summits-height takes an integer in [0, 100]")},
    {"help-summits", no_argument, help(usageSummits)},
    {"genome", required_argument, path(&Opts::genomeFile)},
    {"gc-bias", required_argument, path(&Opts::gcBiasFile)},
    {"gc-window", required_argument, strict(&Opts::gcWindow, &Opts::gcWindowOpt, 1, GX_GC_MAX_WINDOW, ": --gc-window takes an integer in [1, 4096]")},
    {"gc-peaks", required_argument, path(&Opts::gcPeaksFile)},
    {"help-gc", no_argument, help(usageGc)},
    {"motifs", required_argument, path(&Opts::motifsFile)},
    {"motif-hits", required_argument, path(&Opts::motifHitsFile)},
    {"motif-summary", required_argument, path(&Opts::motifSummaryFile)},
    {"motif-pvalue", required_argument, real(&Opts::motifPvalue, &Opts::motifPvalueOpt, [](double p) { return p > 0.0 && p <= 1.0; }, ": --motif-pvalue takes a number in (0, 1]")},
    {"motif-pseudocount", required_argument, real(&Opts::motifPseudo, &Opts::motifPseudoOpt, [](double x) { return x >= 0.0 && std::isfinite(x); }, ": --motif-pseudocount takes a number >= 0")},
    {"help-motifs", no_argument, help(usageMotifs)},
    {"kmers", required_argument, path(&Opts::kmersFile)},
    {"kmer-k", required_argument, strict(&Opts::kmerK, &Opts::kmerKOpt, 1, GX_KMER_MAX_K, ": --kmer-k takes an integer in [1, 12]")},
    {"kmer-flank", required_argument, strict(&Opts::kmerFlank, &Opts::kmerFlankOpt, 0, 1000000000, ": --kmer-flank takes an integer in [0, 1000000000]")},
    {"kmer-top", required_argument, strict(&Opts::kmerTop, &Opts::kmerTopOpt, 0, 16777216, ": --kmer-top takes an integer in [0, 16777216] (0: all)")},
    {"help-kmers", no_argument, help(usageKmers)},
};
const int LONG_BASE = 1000;   // what getopt_long returns for row i: LONG_BASE + i (above every character of the short options)

// The whole command line into `o`: the long options through their rows, the short ones (the reference's getopt string) through
// the switch; the first malformed value of the argv ends the run, then an argument that is no option.
void parseOptions(int argc, char** argv, Opts& o) {
  const char* e = getenv("GENRICH_THREADS");   // --threads N, else GENRICH_THREADS, else up to 16 of the machine's cores
  const unsigned hw = std::thread::hardware_concurrency();
  o.threads = e ? atoi(e) : (int)std::min(16u, hw ? hw : 1u);
  std::vector<option> longOpts;
  for (const LongOpt& r : LONG_OPTS) longOpts.push_back(option{r.name, r.arg, nullptr, r.alias ? r.alias : LONG_BASE + (int)longOpts.size()});
  longOpts.push_back(option{nullptr, 0, nullptr, 0});
  int c;
  while ((c = getopt_long(argc, argv, "ht:c:o:f:k:b:zyw:xjd:De:E:m:s:p:q:a:l:g:rR:XPSL:vV", longOpts.data(), nullptr)) != -1)
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
      case 'h': usage();
      default:
        if (c < LONG_BASE) exit(EXIT_FAILURE);   // (getopt_long has said why)
        LONG_OPTS[c - LONG_BASE].act(o, optarg);
    }
  if (optind < argc) die(argv[optind], ": unknown command-line argument");
}

}  // namespace
