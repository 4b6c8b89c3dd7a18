// host_figures.h -- the figure writers (--counts ... --profile): the frame they share, then one function over the State per figure,
// each with its files and its -v lines, then FIGURES, the table of them.  (a part of genrich_amd.cpp's translation unit)
#pragma once
namespace {

// ---- the frame the writers share --------------------------------------------------------------------------------------------
// The files of one library call: each opened (plain or gzip) where its option was given, NULL where it was not; `write` gets them
// and returns the library's status, which is checked before they are closed.
template <class F>
void writeFiles(State& S, const char* pathA, const char* pathB, F write) {
  Out a, b;
  if (pathA) a = openWrite(pathA, S.o.gzOut);
  if (pathB) b = openWrite(pathB, S.o.gzOut);
  check(S, write(a.f, b.f));
  closeOut(a);
  closeOut(b);
}
// ... and the usual case, one file: nothing happens when its option was not given
template <class F>
void writeFile(State& S, const char* path, F write) {
  if (path) writeFiles(S, path, nullptr, [&](FILE* f, FILE*) { return write(f); });
}

// The sample count that every context agrees on.  count(g, &n) runs on each context -- a pass that can refuse runs here, before a
// file is opened, and a context's refusal carries its own text --; the caller's sentence ends the run when two contexts differ
// or, with `expect`, when one differs from the samples that were read.
template <class F>
int agreedSamples(State& S, const char* sentence, F count, int expect = -1) {
  int nS = expect;
  for (gx_ctx* g : S.devs.ctx) {
    int n = 0;
    check(S, count(g, &n), g);
    if (nS >= 0 && n != nS) die("", sentence);
    nS = n;
  }
  return nS;
}

// a sample as the -v lines name it
std::string sampleLabel(int rep, int ctrl) { return std::string(ctrl ? "control" : "experimental") + " file #" + std::to_string(rep); }

// What a two-call getter fills (first call: the size; second: the data), kept for every sample at once because the formatters take
// all samples: column k of sample i, and per column the pointers of all samples.
struct Columns {
  int nK;
  std::vector<std::vector<uint64_t>> col;
  Columns(int nS, int nK) : nK(nK), col((size_t)nS * nK) {}
  uint64_t* sized(int i, int k, size_t n) {
    col[(size_t)i * nK + k].assign(std::max<size_t>(n, 1), 0);
    return col[(size_t)i * nK + k].data();
  }
  std::vector<const uint64_t*> of(int k) const {
    std::vector<const uint64_t*> p;
    for (size_t i = k; i < col.size(); i += nK) p.push_back(col[i].data());
    return p;
  }
};

std::string countText(long long n) {
  char b[64];
  if (n % 120 == 0) snprintf(b, sizeof b, "%lld", n / 120);
  else snprintf(b, sizeof b, "%.2f", (double)n / 120.0);
  return b;
}
// -v of --counts and --count-regions: per sample the weight counted inside over its total, added over the contexts
template <class Get>
void reportCounted(State& S, int nS, const char* where, const char* ratio, Get get) {
  for (int i = 0; i < nS; i++) {
    long long tot = 0, in = 0;
    int rep = 0, ctrl = 0;
    for (gx_ctx* g : S.devs.ctx) {
      int64_t t = 0, p = 0;
      check(S, get(g, i, &rep, &ctrl, nullptr, 0, &t, &p), g);
      tot += t;
      in += p;
    }
    fprintf(stderr, "  Intervals in %s, %s: %s of %s (%s %f)\n", where, sampleLabel(rep, ctrl).c_str(), countText(in).c_str(),
            countText(tot).c_str(), ratio, tot ? (double)in / (double)tot : 0.0);
  }
}

// ---- the figures ------------------------------------------------------------------------------------------------------------
// --counts: every sample's intervals (its -b lines) counted in the peaks just called, one column per sample in run order --
// for replicate r its treatment, then its control when one was read; with -v the FRiP of each sample
void writeCounts(State& S) {
  const int nS = (int)S.sampleNames.size();
  agreedSamples(S, "--counts: the library kept another number of samples than were read", gx_count_in_peaks, nS);
  writeFile(S, S.o.countsFile, [&](FILE* f) {
    return gx_write_counts_group(S.devs.ctx.data(), (int)S.devs.n(), S.names.data(), nS, S.sampleNames.data(), f);
  });
  if (S.o.verbose) reportCounted(S, nS, "peaks", "FRiP", gx_get_peak_counts);
}

// --peak-signal FILE: every sample's own depth (its -b lines piled up, -E regions not masked) inside the peaks just called: one
// row per narrowPeak line, five columns per sample (gx_write_peak_signal_group); with -v per sample the peaks in which it has no
// depth at all and the peaks whose summit base is also the first base of its own maximum
void writePeakSignal(State& S) {
  writeFile(S, S.o.peakSignalFile, [&](FILE* f) { return gx_write_peak_signal_group(S.devs.ctx.data(), (int)S.devs.n(), S.names.data(), f); });
  if (!S.o.verbose) return;
  for (int i = 0; i < (int)S.sampleNames.size(); i++) {
    size_t total = 0, empty = 0, shared = 0;
    int rep = 0, ctrl = 0;
    for (gx_ctx* g : S.devs.ctx) {
      size_t k = 0;
      check(S, gx_peak_count(g, &k), g);
      std::vector<gx_peak> pk(k);
      std::vector<int64_t> mx(k);
      std::vector<uint32_t> sm(k);
      if (k) check(S, gx_get_peaks(g, pk.data(), k), g);
      check(S, gx_get_peak_signal(g, i, &rep, &ctrl, nullptr, mx.data(), sm.data(), nullptr, nullptr, k), g);
      for (size_t j = 0; j < k; j++) {
        empty += mx[j] == 0;
        shared += sm[j] == pk[j].summit;
      }
      total += k;
    }
    fprintf(stderr, "  Signal in peaks, %s: no depth in %zu of %zu peaks, summit shared in %zu\n", sampleLabel(rep, ctrl).c_str(), empty, total,
            shared);
  }
}

// --summits FILE: every local maximum of the treatments' pooled depth inside the peaks just called that stands out by
// --summits-prominence percent of its height and reaches --summits-height percent of the peak's highest
// (gx_write_summits_group); with -v the peaks, the summits, the peaks with more than one, the most in one peak and the peaks
// without pooled depth (no summit)
void writeSummits(State& S) {
  writeFile(S, S.o.summitsFile, [&](FILE* f) {
    return gx_write_summits_group(S.devs.ctx.data(), (int)S.devs.n(), S.names.data(), S.o.summitsProminence, S.o.summitsHeight, f);
  });
  if (!S.o.verbose) return;
  size_t peaks = 0, summits = 0, multi = 0, most = 0, none = 0;
  for (gx_ctx* g : S.devs.ctx) {
    size_t k = 0, n = 0;
    check(S, gx_peak_count(g, &k), g);
    check(S, gx_peak_summits(g, S.o.summitsProminence, S.o.summitsHeight, &n), g);   // (the count; the writer's pass left the result)
    std::vector<gx_summit> sm(n);
    check(S, gx_get_peak_summits(g, sm.data(), n), g);
    std::vector<size_t> per(k, 0);
    for (const gx_summit& s : sm) per[s.peak]++;
    for (size_t c : per) {
      multi += c > 1;
      none += c == 0;
      most = std::max(most, c);
    }
    peaks += k;
    summits += n;
  }
  fprintf(stderr, "  Summits in peaks: %zu peaks, %zu summits, %zu peaks with more than one, at most %zu in a peak, %zu peaks without pooled depth\n",
          peaks, summits, multi, most, none);
}

// --count-regions BED --region-counts FILE: the same intervals counted in the BED's regions, which may overlap and come in any
// order; exactly one output row per BED line, in the BED's order, so that the files of two runs line up.  The BED is read with
// -E's rules (loadBED); a 4th column names the row, further columns are ignored (a narrowPeak file is valid input).
// (--profile reads its BED by the same rules; there column 6 gives the strand: + and - as given, . or no column 6 means +)
void loadRegionRows(State& S, const char* fn, std::vector<RegionRow>& rows, std::vector<int>* strands) {
  std::vector<char> line(65520);
  In in;
  openRead(in, fn, S.threads.sam.inflate);
  while (in.gets(line.data(), (int)line.size())) {
    // in the reference's order (5203-5213): a field is converted as soon as it has been cut off, and a missing one is reported
    // with what strtok has left of the line, i.e. the name
    char* name = strtok(line.data(), "\t");
    if (!name) die(line.data(), ": poorly formatted BED record");
    char* a = strtok(nullptr, "\t");
    if (!a) die(line.data(), ": poorly formatted BED record");
    const int p0 = getInt(a);
    char* b = strtok(nullptr, "\t\n");
    if (!b) die(line.data(), ": poorly formatted BED record");
    const int p1 = getInt(b);
    if (p1 <= p0 || p0 < 0 || p1 < 0) {
      char msg[512];
      snprintf(msg, sizeof msg, "%s, %d - %d", name, p0, p1);
      die(msg, ": poorly formatted BED record");
    }
    const char* rn = strtok(nullptr, "\t\n");
    rows.push_back(RegionRow{name, rn ? rn : "", (uint32_t)p0, (uint32_t)p1, rn != nullptr});
    if (!strands) continue;
    const char* st = rn && strtok(nullptr, "\t\n") ? strtok(nullptr, "\t\n") : nullptr;   // (behind the score)
    if (st && strcmp(st, "+") && strcmp(st, "-") && strcmp(st, ".")) {
      char msg[512];
      snprintf(msg, sizeof msg, "%s, %d - %d, strand %s", rows.back().chrom.c_str(), p0, p1, st);
      die(msg, ": poorly formatted BED record");
    }
    strands->push_back(st && st[0] == '-' ? -1 : 1);
  }
  checkIn(in);
  in.close();
}
// -E FILE[,FILE...] (loadBED 5187-5238): the same three fields of every line of every file
void loadBED(State& S, const char* files) {
  std::string list(files);
  std::vector<RegionRow> rows;
  char* endFn = nullptr;  // (strtok_r as in the reference: the lines are cut up with strtok inside the loop)
  for (char* fn = strtok_r(list.data(), ", ", &endFn); fn; fn = strtok_r(nullptr, ", ", &endFn)) loadRegionRows(S, fn, rows, nullptr);
  for (const RegionRow& r : rows) S.xbed.push_back(BedRec{r.chrom, {r.start, r.end}});
}
void writeRegionCounts(State& S) {
  const int nS = (int)S.sampleNames.size();
  ChromNames names(S.chrom);
  std::vector<gx_region> reg(S.regions.size());
  std::vector<const char*> regNames(S.regions.size());
  for (size_t k = 0; k < S.regions.size(); k++) {
    const RegionRow& r = S.regions[k];
    reg[k] = gx_region{names.of(r.chrom), r.start, r.end};
    regNames[k] = r.named ? r.name.c_str() : nullptr;
  }
  agreedSamples(S, "--count-regions: the library kept another number of samples than were read",
                [&](gx_ctx* g, int* n) { return gx_count_in_regions(g, reg.data(), reg.size(), n); }, nS);
  writeFile(S, S.o.regionCountsFile, [&](FILE* f) {
    return gx_write_region_counts_group(S.devs.ctx.data(), (int)S.devs.n(), names.all.data(), reg.data(), regNames.data(), reg.size(), nS,
                                        S.sampleNames.data(), f);
  });
  if (S.o.verbose) reportCounted(S, nS, "regions", "fraction", gx_get_region_counts);
}

// the samples closed on the first context, as the outputs per sample name them: t<rep> for a treatment, c<rep> for a control
// that was read; from the coverage's samples, or the profile's (the same samples in the same order)
struct ClosedSamples {
  std::vector<std::string> labels;
  std::vector<const char*> names;   // the labels, for the library (good while `labels` is not copied or grown)
  std::vector<int> reps, ctrls;
  int n() const { return (int)labels.size(); }
};
ClosedSamples closedSamples(State& S, bool profile = false) {
  gx_ctx* g0 = S.devs.ctx[0];
  int nS = 0;
  check(S, profile ? gx_profile_samples(g0, &nS) : gx_coverage_samples(g0, &nS), g0);
  ClosedSamples L;
  L.labels.reserve((size_t)nS);   // (no label moves after `names` points at it)
  for (int i = 0; i < nS; i++) {
    int rep = 0, ctrl = 0;
    check(S, profile ? gx_get_profile(g0, i, &rep, &ctrl, nullptr, nullptr, 0, 0) : gx_get_coverage(g0, i, 0, &rep, &ctrl, nullptr, 0), g0);
    L.labels.push_back((ctrl ? "c" : "t") + std::to_string(rep));
    L.names.push_back(L.labels.back().c_str());
    L.reps.push_back(rep);
    L.ctrls.push_back(ctrl);
  }
  return L;
}

// the smallest finite entry above the diagonal of an nS x nS matrix: its row and column, (-1, -1) when there is none
std::pair<int, int> leastAlike(const std::vector<double>& r, int nS) {
  int li = -1, lj = -1;
  for (int i = 0; i < nS; i++)
    for (int j = i + 1; j < nS; j++)
      if (r[(size_t)i * nS + j] == r[(size_t)i * nS + j] && (li < 0 || r[(size_t)i * nS + j] < r[(size_t)li * nS + lj])) { li = i; lj = j; }
  return {li, lj};
}

// --coverage PREFIX: each sample's pileup in bins, one bedGraph file per sample -- PREFIX.t<rep>.bedgraph for a treatment,
// PREFIX.c<rep>.bedgraph for a control that was read (.gz behind it with -z); with -v the mean of each track
void writeCoverage(State& S) {
  const Opts& o = S.o;
  const int nChrom = (int)S.names.size();
  const int nS = agreedSamples(S, "--coverage: the devices closed different numbers of samples", gx_coverage_samples);
  const ClosedSamples L = closedSamples(S);
  std::vector<int64_t> sums;
  for (int i = 0; i < nS; i++) {
    const std::string path = std::string(o.coveragePrefix) + "." + L.labels[i] + ".bedgraph" + (o.gzOut ? ".gz" : "");
    writeFile(S, path.c_str(), [&](FILE* f) {
      return gx_write_coverage_group(S.devs.ctx.data(), S.devs.owner.data(), i, S.names.data(), nChrom, o.coverageScale, f);
    });
    if (!o.verbose) continue;
    double total = 0.0;   // (sum120 / 120 over the chromosomes written)
    unsigned long long bp = 0;
    for (int c = 0; c < nChrom; c++) {
      gx_ctx* g = S.devs.ctx[S.devs.owner[c]];
      size_t n = 0;
      uint32_t len = 0;
      check(S, gx_coverage_bin_count(g, c, &n), g);
      if (!n) continue;
      check(S, gx_coverage_layout(g, c, nullptr, &len), g);
      sums.assign(n, 0);
      check(S, gx_get_coverage(g, i, c, nullptr, nullptr, sums.data(), n), g);
      __int128 sum = 0;
      for (int64_t v : sums) sum += v;
      total += (double)sum / 120.0;
      bp += len;
    }
    fprintf(stderr, "  Coverage, %s: mean %f over %llu bp\n", sampleLabel(L.reps[i], L.ctrls[i]).c_str(), bp ? total / (double)bp : 0.0, bp);
  }
}

// --correlation / --spearman: the matrix from the added sums as a TSV labelled t<rep> / c<rep> like --coverage's files (.gz'd with
// -z); with -v, behind what `head` prints of the figure's own, the least alike pair
template <class Head>
void writeMatrix(State& S, const char* path, const ClosedSamples& L, uint64_t n, uint64_t zeros, int skipZeros, const std::vector<gx_u128>& sum,
                 const std::vector<gx_u128>& gram, const char* coefficient, Head head) {
  const int nS = L.n();
  writeFile(S, path, [&](FILE* f) { return gx_format_correlation(f, nS, L.names.data(), n, zeros, sum.data(), gram.data(), skipZeros); });
  if (!S.o.verbose) return;
  std::vector<double> r((size_t)nS * nS);
  check(S, gx_correlation_matrix(nS, n, zeros, sum.data(), gram.data(), skipZeros, r.data()));
  const auto [li, lj] = leastAlike(r, nS);
  head();
  if (li >= 0) fprintf(stderr, "; smallest %s %f (%s, %s)\n", coefficient, r[(size_t)li * nS + lj], L.names[li], L.names[lj]);
  else fprintf(stderr, "; no pair with a correlation\n");
}

// --correlation FILE: the Pearson matrix of the samples' coverage bins (all bins, or with --corr-skip-zeros those that are not
// zero in every sample); with -v the bins and the least alike pair
void writeCorrelation(State& S) {
  const ClosedSamples L = closedSamples(S);
  const int nS = L.n();
  // one pass per context; the matrix is formatted, and with -v searched, from the added sums
  std::vector<gx_u128> sum((size_t)nS), gram((size_t)nS * nS);
  uint64_t bins = 0, zeros = 0;
  check(S, gx_coverage_gram_group(S.devs.ctx.data(), (int)S.devs.n(), nS, &bins, &zeros, sum.data(), gram.data()));
  writeMatrix(S, S.o.correlationFile, L, bins, zeros, S.o.corrSkipZeros ? 1 : 0, sum, gram, "r",
              [&] { fprintf(stderr, "  Correlation: %llu bins, %llu all zero", (unsigned long long)bins, (unsigned long long)zeros); });
}

// --spearman FILE: the Spearman matrix of the same bins (with --corr-skip-zeros: of those that are not zero in every sample, taken
// out before ranking), --correlation's TSV; with -v the bins ranked, the most distinct values a sample has and the least alike pair
void writeSpearman(State& S) {
  const ClosedSamples L = closedSamples(S);
  const int nS = L.n();
  // every context's value tables, one ranking over all of them, one pass per context over its rank rows; the sums are added
  std::vector<gx_u128> sum((size_t)nS), gram((size_t)nS * nS);
  std::vector<uint64_t> distinct((size_t)nS);
  uint64_t ranked = 0;
  check(S, gx_coverage_spearman_group(S.devs.ctx.data(), (int)S.devs.n(), nS, S.o.corrSkipZeros ? 1 : 0, &ranked, sum.data(), gram.data(),
                                      distinct.data()));
  writeMatrix(S, S.o.spearmanFile, L, ranked, 0, 0, sum, gram, "rho", [&] {
    fprintf(stderr, "  Spearman: %llu bins ranked, at most %llu distinct values a sample", (unsigned long long)ranked,
            nS ? (unsigned long long)*std::max_element(distinct.begin(), distinct.end()) : 0ull);
  });
}

// --fingerprint FILE [--fingerprint-metrics FILE]: each sample's bins reduced to value classes (one pass per context, added),
// the Lorenz curve's points per sample and non-empty class as a TSV labelled t<rep> / c<rep> like --correlation's, and the
// figures made of them (zero fraction, area, Gini, elbow, the divergence from the replicate's control); with -v the figures
// on stderr too
void writeFingerprint(State& S) {
  const Opts& o = S.o;
  gx_ctx* g0 = S.devs.ctx[0];
  const ClosedSamples L = closedSamples(S);
  const int nS = L.n();
  const std::vector<const char*>& names = L.names;
  std::vector<int> ctrlOf((size_t)nS, -1);   // a treatment's control: the control sample of the same replicate
  for (int i = 0; i < nS; i++)
    for (int j = 0; j < nS && !L.ctrls[i]; j++)
      if (L.ctrls[j] && L.reps[j] == L.reps[i]) ctrlOf[i] = j;
  std::vector<uint64_t> count((size_t)nS * GX_FP_NC), sum((size_t)nS * GX_FP_NC);
  check(S, gx_coverage_fingerprint_group(S.devs.ctx.data(), (int)S.devs.n(), nS, nullptr, count.data(), sum.data()), g0);
  writeFile(S, o.fingerprintFile, [&](FILE* f) { return gx_format_fingerprint(f, nS, names.data(), count.data(), sum.data()); });
  writeFile(S, o.fingerprintMetricsFile, [&](FILE* f) { return gx_format_fingerprint_metrics(f, nS, names.data(), count.data(), sum.data(), ctrlOf.data()); });
  if (!o.verbose) return;
  std::vector<gx_fp_metrics> m((size_t)nS);
  check(S, gx_fingerprint_metrics(nS, count.data(), sum.data(), ctrlOf.data(), m.data()), g0);
  for (int i = 0; i < nS; i++)
    fprintf(stderr, "  Fingerprint %s: zero fraction %f, auc %f, gini %f, elbow at %f of the bins (gap %f), jsd to control %f\n", names[i],
            m[i].zero_fraction, m[i].auc, m[i].gini, m[i].elbow_bins, m[i].elbow_gap, m[i].jsd_control);
}

// --complexity FILE [--complexity-hist FILE]: each sample's intervals (its -b lines) as observations of (chromosome, start, end)
// keys, counted on the device (one pass per context and sample, added): N, D, the duplication histogram and the figures made
// of it (NRF, PBC1, PBC2, the duplicate fraction, the estimated library size, the complexity curve), one row per sample labelled
// t<rep> / c<rep>; with -v the main figures on stderr too
void writeComplexity(State& S) {
  const Opts& o = S.o;
  gx_ctx* const* ctxs = S.devs.ctx.data();
  const int nCtx = (int)S.devs.n();
  const int nS = agreedSamples(S, "--complexity: the devices kept different numbers of samples", gx_complexity);
  std::vector<int> rep((size_t)nS), ctrl((size_t)nS);
  std::vector<uint64_t> N((size_t)nS), D((size_t)nS);
  std::vector<size_t> np((size_t)nS);
  Columns cols(nS, 2);   // multiplicities, keys
  for (int i = 0; i < nS; i++) {
    check(S, gx_complexity_group(ctxs, nCtx, i, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &np[i]));
    uint64_t *mult = cols.sized(i, 0, np[i]), *keys = cols.sized(i, 1, np[i]);
    check(S, gx_complexity_group(ctxs, nCtx, i, &rep[i], &ctrl[i], &N[i], &D[i], mult, keys, np[i], nullptr));
  }
  const std::vector<const uint64_t*> pm = cols.of(0), pk = cols.of(1);
  writeFile(S, o.complexityFile, [&](FILE* f) { return gx_format_complexity(f, nS, rep.data(), ctrl.data(), N.data(), D.data(), pm.data(), pk.data(), np.data()); });
  writeFile(S, o.complexityHistFile, [&](FILE* f) { return gx_format_complexity_hist(f, nS, rep.data(), ctrl.data(), pm.data(), pk.data(), np.data()); });
  if (!o.verbose) return;
  for (int i = 0; i < nS; i++) {
    gx_cpx_metrics m;
    check(S, gx_complexity_metrics(N[i], D[i], pm[i], pk[i], np[i], &m));
    fprintf(stderr, "  Library complexity, %s: %llu intervals, %llu distinct (NRF %f, PBC1 %f, PBC2 %f, estimated library size %.0f)\n",
            sampleLabel(rep[i], ctrl[i]).c_str(), (unsigned long long)N[i], (unsigned long long)D[i], m.nrf, m.pbc1, m.pbc2, m.library_size);
  }
}

// --lengths FILE / --lengths-metrics FILE / --chrom-stats FILE: each sample's intervals (its -b lines) by length and by
// chromosome, counted on the device (one pass per context and sample, added): one row per sample and occurring length, one row
// of figures per sample (mean, sd, quantiles, mode, the shares of the --lengths-cuts classes), one row per chromosome with each
// sample's intervals, weight, share and mean depth; labelled t<rep> / c<rep>.  With -j the intervals are cut-site windows, not
// fragments, and the header says so.  With -v the median and mode, the shares and the fullest chromosome on stderr too
void writeIntervalStats(State& S) {
  const Opts& o = S.o;
  gx_ctx* const* ctxs = S.devs.ctx.data();
  const int nCtx = (int)S.devs.n();
  const size_t nC = S.names.size();
  const int nS = agreedSamples(S, "--lengths: the devices kept different numbers of samples", gx_interval_stats);
  std::vector<int> rep((size_t)nS), ctrl((size_t)nS);
  std::vector<uint64_t> nInv((size_t)nS), wInv((size_t)nS);
  std::vector<size_t> np((size_t)nS);
  Columns cols(nS, 6);   // per length: the length, its intervals, their weight; per chromosome: intervals, weight, bases
  for (int i = 0; i < nS; i++) {
    check(S, gx_interval_stats_group(ctxs, nCtx, i, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &np[i], nullptr, nullptr, nullptr, nullptr,
                                     nullptr, 0));
    uint64_t* a[6];
    for (int k = 0; k < 6; k++) a[k] = cols.sized(i, k, k < 3 ? np[i] : nC);
    check(S, gx_interval_stats_group(ctxs, nCtx, i, &rep[i], &ctrl[i], a[0], a[1], a[2], np[i], nullptr, &nInv[i], &wInv[i], a[3], a[4], a[5], nC));
  }
  const std::vector<const uint64_t*> pl = cols.of(0), pn = cols.of(1), pw = cols.of(2), pcn = cols.of(3), pcw = cols.of(4), pcb = cols.of(5);
  const uint64_t* cuts = o.lengthsCuts.data();
  const int nCuts = (int)o.lengthsCuts.size();
  writeFile(S, o.lengthsFile, [&](FILE* f) {
    return gx_format_lengths(f, nS, rep.data(), ctrl.data(), pl.data(), pn.data(), pw.data(), np.data(), nInv.data(), wInv.data(), o.atacOpt ? 1 : 0);
  });
  writeFile(S, o.lengthsMetricsFile, [&](FILE* f) {
    return gx_format_lengths_metrics(f, nS, rep.data(), ctrl.data(), pl.data(), pn.data(), pw.data(), np.data(), cuts, nCuts);
  });
  writeFile(S, o.chromStatsFile, [&](FILE* f) {
    std::vector<uint32_t> lens;
    for (const Chrom& ch : S.chrom) lens.push_back(ch.len);
    return gx_format_chrom_stats(f, S.names.data(), lens.data(), (int)nC, nS, rep.data(), ctrl.data(), pcn.data(), pcw.data(), pcb.data());
  });
  if (!o.verbose) return;
  for (int i = 0; i < nS; i++) {
    gx_len_metrics m;
    check(S, gx_lengths_metrics(pl[i], pn[i], pw[i], np[i], cuts, nCuts, &m));
    size_t top = 0;
    unsigned __int128 W = 0;
    for (size_t c = 0; c < nC; c++) {
      W += pcw[i][c];
      if (pcw[i][c] > pcw[i][top]) top = c;
    }
    fprintf(stderr, "  Interval lengths%s, %s: %llu intervals, median %llu, mode %llu; shares", o.atacOpt ? " (cut-site windows)" : "",
            sampleLabel(rep[i], ctrl[i]).c_str(), (unsigned long long)m.n, (unsigned long long)m.median, (unsigned long long)m.mode);
    for (int k = 0; k <= nCuts; k++) fprintf(stderr, " %f", m.n ? m.share[k] : 0.0);
    fprintf(stderr, "; most on %s (%f)\n", nC ? S.names[top] : "-", W ? (double)pcw[i][top] / (double)W : 0.0);
  }
}

// --genome FASTA: every sequence the run knows goes to the context that owns its chromosome, staging buffer by staging buffer
// (host_genome.h strips it, gx_push_sequence packs it on the device).  A sequence the run does not know is skipped; one whose
// length differs from the header's LN ends the run with both lengths; a chromosome of the run that the FASTA lacks stays
// unknown, with one warning each under -v.  Plain text through a mapping; gzip and BGZF through the input stream's inflaters.
struct GenomeSink {
  State& S;
  ChromNames names;
  std::vector<uint8_t> seen;
  int c = -1;
  bool tooLong = false;
  uint64_t nSeq = 0, nBases = 0;
  std::string err;
  explicit GenomeSink(State& s) : S(s), names(s.chrom), seen(s.chrom.size(), 0) {}
  bool lengths(uint64_t fasta) {
    err = S.chrom[c].name + ": the sequence in " + S.o.genomeFile + " has " + std::to_string(fasta) + (tooLong ? " bases or more" : " bases") +
          ", the alignment files' header says " + std::to_string(S.chrom[c].len);
    return false;
  }
  bool begin(const std::string& name) {
    const auto it = names.idx.find(name);
    if (it == names.idx.end() || S.chrom[it->second].skip) return false;
    c = (int)it->second;
    if (seen[c]) {
      err = name + ": twice in " + S.o.genomeFile;
      c = -1;
      return true;   // (bases() stops the reading)
    }
    seen[c] = 1;
    tooLong = false;
    nSeq++;
    return true;
  }
  bool bases(uint64_t first, const char* p, size_t n) {
    if (c < 0) return false;
    const uint64_t len = S.chrom[c].len;
    if (first + n > len) {   // (more may follow: end() knows the length)
      tooLong = true;
      return lengths(first + n);
    }
    if (n % 64 && first + n != len) return lengths(first + n);   // (a staging buffer that is not full is the sequence's last)
    gx_ctx* g = S.devs.ctx[S.devs.owner[c]];
    const int rc = gx_push_sequence(g, c, first, p, n);
    if (rc) {
      err = gx_last_error(g);
      if (err.empty()) err = gx_strerror(rc);
      return false;
    }
    nBases += n;
    return true;
  }
  bool end(uint64_t length) {
    if (c < 0) return false;
    return length == S.chrom[c].len ? true : lengths(length);
  }
};

void loadGenome(State& S) {
  const Opts& o = S.o;
  const auto t0 = std::chrono::steady_clock::now();
  for (gx_ctx* g : S.devs.ctx) check(S, gx_set_genome(g, 1), g);
  if (o.motifsFile || o.kmersFile)   // (the scan and the k-mers need the bases themselves: the third vector)
    for (gx_ctx* g : S.devs.ctx) check(S, gx_set_genome_bases(g, 1), g);
  if (o.motifsFile)   // (... and the motifs with it)
    for (gx_ctx* g : S.devs.ctx) check(S, gx_set_motifs(g, S.motifRecs.data(), (int)S.motifRecs.size(), S.motifScores.data()), g);
  GenomeSink sink(S);
  const size_t chunk = (size_t)1 << 22;
  unsigned char magic[2] = {0, 0};
  {
    FILE* f = fopen(o.genomeFile, "rb");
    if (!f) die(o.genomeFile, ": cannot open file for reading");
    const size_t k = fread(magic, 1, 2, f);
    fclose(f);
    if (!k) die(o.genomeFile, ": --genome: an empty file");
  }
  bool ok;
  if (magic[0] == 0x1f && magic[1] == 0x8b) {
    In in;
    openRead(in, o.genomeFile, S.threads.sam.inflate);
    ok = gxhost::genome_read_stream(in, o.genomeFile, chunk, sink, &sink.err);
    checkIn(in);
    in.close();
  } else {
    ok = gxhost::genome_read_plain(o.genomeFile, chunk, sink, &sink.err);
  }
  if (!ok) die("--genome: ", sink.err.c_str());
  if (!o.verbose) return;
  for (size_t i = 0; i < S.chrom.size(); i++)
    if (!sink.seen[i] && !S.chrom[i].skip)
      fprintf(stderr, "Warning! %s is not in %s: its bases are unknown to --gc-bias and --gc-peaks\n", S.chrom[i].name.c_str(), o.genomeFile);
  uint64_t gc = 0, acgt = 0;
  for (gx_ctx* g : S.devs.ctx) {
    uint64_t a = 0, b = 0;
    check(S, gx_genome_info(g, nullptr, &a, &b), g);   // (drains the device: the time below is the whole way)
    gc += a;
    acgt += b;
  }
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  fprintf(stderr, "Genome %s: %llu sequences, %llu bases (%llu known, %llu G or C) in %.3f s\n", o.genomeFile, (unsigned long long)sink.nSeq,
          (unsigned long long)sink.nBases, (unsigned long long)acgt, (unsigned long long)gc, sec);
}

// --gc-bias FILE: each sample's intervals (its -b lines) by the GC content of the --gc-window bases from their start, over the
// genome's windows of that content, counted on the device (one pass per context and distinct set of chromosomes for the
// genome's side, one per context and sample for the sample's; added): per sample a `#` line and 101 rows, labelled t<rep> /
// c<rep>.  -E regions are not masked on either side.  With -v the mean window GC of the sample's intervals and of the genome, and
// the least and the greatest ratio among the classes that hold at least 1 % of the windows
void writeGcBias(State& S) {
  const Opts& o = S.o;
  gx_ctx* const* ctxs = S.devs.ctx.data();
  const int nCtx = (int)S.devs.n(), W = o.gcWindow;
  const int nS = agreedSamples(S, "--gc-bias: the devices kept different numbers of samples", [&](gx_ctx* g, int* n) { return gx_gc_bias(g, W, n); });
  std::vector<int> rep((size_t)nS), ctrl((size_t)nS);
  std::vector<uint64_t> fUn((size_t)nS), nUn((size_t)nS), wUn((size_t)nS);
  Columns cols(nS, 3);   // per window class: the genome's windows, the sample's intervals, their weight
  for (int i = 0; i < nS; i++) {
    uint64_t* a[3];
    for (int k = 0; k < 3; k++) a[k] = cols.sized(i, k, (size_t)W + 1);
    check(S, gx_gc_bias_group(ctxs, nCtx, i, &rep[i], &ctrl[i], nullptr, a[0], &fUn[i], a[1], a[2], &nUn[i], &wUn[i], (size_t)W + 1));
  }
  const std::vector<const uint64_t*> pF = cols.of(0), pN = cols.of(1), pW = cols.of(2);
  writeFile(S, o.gcBiasFile, [&](FILE* f) {
    return gx_format_gc_bias(f, nS, rep.data(), ctrl.data(), W, pF.data(), fUn.data(), pN.data(), pW.data(), nUn.data(), wUn.data());
  });
  if (!o.verbose) return;
  for (int i = 0; i < nS; i++) {
    gx_gc_metrics_t m;
    check(S, gx_gc_metrics(W, pF[i], fUn[i], pN[i], pW[i], nUn[i], wUn[i], &m));
    fprintf(stderr, "  GC bias, %s: mean window GC ", sampleLabel(rep[i], ctrl[i]).c_str());
    if (std::isnan(m.mean_gc_sample)) fprintf(stderr, "NA");
    else fprintf(stderr, "%f", m.mean_gc_sample);
    if (std::isnan(m.mean_gc_genome)) fprintf(stderr, " (genome NA)");
    else fprintf(stderr, " (genome %f)", m.mean_gc_genome);
    if (m.ratio_min_class < 0) fprintf(stderr, ", ratio NA\n");
    else fprintf(stderr, ", ratio %f at %d %% to %f at %d %% GC\n", m.ratio_min, m.ratio_min_class, m.ratio_max, m.ratio_max_class);
  }
}

// --gc-peaks FILE: the rows of --counts (the same peak_N), then the peak's length, its known bases, its G or C among them and
// their share, by rank differences on the context that owns the chromosome (gx_write_gc_peaks_group)
void writeGcPeaks(State& S) {
  writeFile(S, S.o.gcPeaksFile, [&](FILE* f) { return gx_write_gc_peaks_group(S.devs.ctx.data(), (int)S.devs.n(), S.names.data(), f); });
}

// --motifs FILE: the JASPAR matrices (host_motifs.h) to scores and thresholds (gx_motif_pssm, gx_motif_threshold: host only), and
// to every context.  A matrix the reader or the library refuses ends the run with its ID and the sentence; a motif that cannot
// hit at --motif-pvalue stays in the run with one warning under -v and NA for its p.
void loadMotifs(State& S) {
  const Opts& o = S.o;
  std::string err;
  if (!gxhost::motifs_read_plain(o.motifsFile, S.motifs, &err)) die("--motifs: ", err.c_str());
  size_t at = 0;
  for (const gxhost::MotifRec& m : S.motifs) at += 4 * (size_t)m.width;
  S.motifScores.assign(at, 0);
  at = 0;
  for (const gxhost::MotifRec& m : S.motifs) {
    char why[160] = "";
    int32_t t = 0;
    double p = 0.0;
    int unreachable = 0;
    if (gx_motif_pssm(m.counts.data(), (int)m.width, o.motifPseudo, S.motifScores.data() + at, nullptr, nullptr, why, sizeof why) != GX_OK)
      die("--motifs: ", (m.id + ": " + (why[0] ? why : "a matrix the library refuses")).c_str());
    check(S, gx_motif_threshold(S.motifScores.data() + at, (int)m.width, o.motifPvalue, &t, nullptr, nullptr, &p, &unreachable));
    if (unreachable && o.verbose)
      fprintf(stderr, "Warning! motif %s cannot hit at --motif-pvalue %g: even its best score has more than that share of the %u-mers\n", m.id.c_str(),
              o.motifPvalue, m.width);
    S.motifRecs.push_back(gx_motif{m.width, (uint32_t)at, t});
    S.motifP.push_back(unreachable ? std::nan("") : p);
    at += 4 * (size_t)m.width;
  }
  if (o.verbose) fprintf(stderr, "Motifs %s: %zu matrices, p-value %g, pseudocount %g\n", o.motifsFile, S.motifs.size(), o.motifPvalue, o.motifPseudo);
}

// --motif-hits FILE / --motif-summary FILE: the motifs in the called peaks (k_motif_scan on the context that owns the
// chromosome; the same peak_N as -o) and, for the summary, counted over the whole genome too.  With -v the hits, the peaks with
// any, the three most enriched motifs and the time of the genome pass
void writeMotifs(State& S) {
  const Opts& o = S.o;
  gx_ctx* const* ctxs = S.devs.ctx.data();
  const int nCtx = (int)S.devs.n(), nM = (int)S.motifs.size();
  std::vector<const char*> ids, mnames;
  for (const gxhost::MotifRec& m : S.motifs) {
    ids.push_back(m.id.c_str());
    mnames.push_back(m.name.c_str());
  }
  // (one call for both files: the peaks are scanned once, the genome once and only for the summary)
  std::vector<uint64_t> cp((size_t)3 * nM + 1, 0), cg((size_t)3 * nM + 1, 0);
  gx_motif_report rep{};
  writeFiles(S, o.motifHitsFile, o.motifSummaryFile, [&](FILE* hits, FILE* summary) {
    return gx_write_motifs_group(ctxs, nCtx, S.names.data(), S.motifRecs.data(), ids.data(), mnames.data(), S.motifP.data(), nM, hits, summary, cp.data(),
                                 cg.data(), &rep);
  });
  if (!o.verbose) return;
  fprintf(stderr, "Motif hits: %llu in %llu peaks\n", (unsigned long long)rep.hits, (unsigned long long)rep.peaks_with_hit);
  if (!o.motifSummaryFile) return;
  std::vector<std::pair<double, int>> enr;
  for (int m = 0; m < nM; m++) {
    const double hp = (double)(cp[(size_t)nM + m] + cp[(size_t)2 * nM + m]), hg = (double)(cg[(size_t)nM + m] + cg[(size_t)2 * nM + m]);
    if (hg > 0 && cp[m]) enr.push_back({(hp * (double)cg[m]) / (hg * (double)cp[m]), m});
  }
  std::sort(enr.begin(), enr.end(), [](const std::pair<double, int>& x, const std::pair<double, int>& y) { return x.first != y.first ? x.first > y.first : x.second < y.second; });
  for (size_t k = 0; k < enr.size() && k < 3; k++)
    fprintf(stderr, "  Motif %s (%s): enrichment %f\n", S.motifs[enr[k].second].id.c_str(), S.motifs[enr[k].second].name.c_str(), enr[k].first);
  fprintf(stderr, "  Motif summary: the peaks in %.3f s, the genome pass in %.3f s\n", rep.peaks_seconds, rep.genome_seconds);
}

// --kmers FILE [--kmer-k K] [--kmer-flank N] [--kmer-top N]: every K-mer of the called peaks (whole, or N bases to either side of
// the summit) counted on the device that owns the chromosome, and of the whole genome (k_kmer_count); the strands collapsed, the
// enrichment and the z-score per canonical K-mer, the N highest.  With -v the windows, the three top K-mers and the genome pass's
// seconds
void writeKmers(State& S) {
  const Opts& o = S.o;
  gx_kmer_report rep{};
  writeFile(S, o.kmersFile, [&](FILE* f) {
    return gx_write_kmers_group(S.devs.ctx.data(), (int)S.devs.n(), o.kmerK, o.kmerFlankOpt ? o.kmerFlank : -1, o.kmerTop, f, &rep);
  });
  if (!o.verbose) return;
  fprintf(stderr, "K-mers (k = %d): %llu windows in %llu regions of the peaks, %llu in the genome, %llu canonical k-mers counted\n", o.kmerK,
          (unsigned long long)rep.windows_peaks, (unsigned long long)rep.regions_counted, (unsigned long long)rep.windows_genome,
          (unsigned long long)rep.kmers_counted);
  for (int i = 0; i < rep.n_top; i++) {
    char s[GX_KMER_MAX_K + 1];
    for (int j = 0; j < o.kmerK; j++) s[j] = "ACGT"[(rep.top_code[i] >> (2 * (o.kmerK - 1 - j))) & 3u];
    s[o.kmerK] = '\0';
    if (std::isnan(rep.top_z[i])) fprintf(stderr, "  K-mer %s: z NA\n", s);
    else fprintf(stderr, "  K-mer %s: z %.4f\n", s, rep.top_z[i]);
  }
  fprintf(stderr, "  K-mers: the peaks in %.3f s, the genome pass in %.3f s\n", rep.peaks_seconds, rep.genome_seconds);
}

// --xcor FILE / --xcor-metrics FILE: the strand cross-correlation of each sample's 5' ends, counted on the device when the
// sample was closed (one pass per context, added): the curve, one row per sample and shift with the exact pair count and r, and
// one row of figures per sample (fragment length, NSC, RSC), labelled t<rep> / c<rep>.  With -v the figures on stderr too, and
// for a library whose unpaired alignments gave tags, with no extension chosen, the length to extend them to
void writeXcor(State& S) {
  const Opts& o = S.o;
  gx_ctx* const* ctxs = S.devs.ctx.data();
  const int nCtx = (int)S.devs.n();
  const int nS = agreedSamples(S, "--xcor: the devices closed different numbers of samples", gx_xcor_samples);
  writeFiles(S, o.xcorFile, o.xcorMetricsFile, [&](FILE* curve, FILE* metrics) { return gx_write_xcor_group(ctxs, nCtx, o.xcorReadLen, curve, metrics); });
  if (!o.verbose) return;
  std::vector<uint64_t> n11((size_t)(o.xcorHi - o.xcorLo + 1));
  for (int i = 0; i < nS; i++) {
    int rep = 0, ctrl = 0;
    uint64_t N = 0, nP = 0, nM = 0;
    check(S, gx_xcor_group(ctxs, nCtx, i, &rep, &ctrl, &N, &nP, &nM, nullptr, nullptr, nullptr, n11.data(), n11.size()));
    gx_xcor_metrics_t m;
    check(S, gx_xcor_metrics(N, nP, nM, o.xcorLo, o.xcorHi, n11.data(), o.xcorReadLen, &m));
    fprintf(stderr, "  Strand cross-correlation, %s: fragment length ", sampleLabel(rep, ctrl).c_str());
    if (m.has_frag) fprintf(stderr, "%d", m.fragment_length);
    else fprintf(stderr, "NA");
    auto put = [](const char* name, double v) {
      if (std::isnan(v)) fprintf(stderr, ", %s NA", name);
      else fprintf(stderr, ", %s %f", name, v);
    };
    put("NSC", m.nsc);
    put("RSC", m.rsc);
    fprintf(stderr, "\n");
    // (Genrich extends unpaired alignments to a given length with -w N, to the pairs' average with -x: a single-end library has
    // no pairs, and this is the length either would want)
    if (m.has_frag && !ctrl && S.unpairedTags && !o.extendOpt && !o.avgExtOpt)
      fprintf(stderr, "  suggested -x %d (unpaired alignments extended to the estimated fragment length: -w %d)\n", m.fragment_length, m.fragment_length);
  }
}

// --depth FILE / --depth-metrics FILE: the distribution of per-base depth of each sample's pileup, taken on the device when the
// sample was closed (one pass per context, added): one row per sample and non-empty whole depth, and one row of figures per
// sample (bases, covered, mean, sd, min, quartiles, percentiles, max, the fractions at 1x .. 100x), labelled t<rep> / c<rep>; with
// -v the mean, the median and the share covered on stderr too
void writeDepth(State& S) {
  const Opts& o = S.o;
  gx_ctx* const* ctxs = S.devs.ctx.data();
  const int nCtx = (int)S.devs.n();
  int nS = 0;
  check(S, gx_depth_samples(S.devs.ctx[0], &nS));
  if (nS < 1) die("", "--depth: no sample was closed");
  writeFiles(S, o.depthFile, o.depthMetricsFile, [&](FILE* depth, FILE* metrics) { return gx_write_depth_group(ctxs, nCtx, depth, metrics); });
  if (!o.verbose) return;
  std::vector<uint64_t> bases(GX_DEPTH_BOUND), rsum(GX_DEPTH_BOUND), rsq(GX_DEPTH_BOUND), deepV, deepBases;
  for (int i = 0; i < nS; i++) {
    size_t n = 0;
    check(S, gx_depth_group(ctxs, nCtx, i, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n));
    deepV.assign(std::max<size_t>(n, 1), 0);
    deepBases.assign(std::max<size_t>(n, 1), 0);
    gx_depth_hist h;
    check(S, gx_depth_group(ctxs, nCtx, i, &h, bases.data(), rsum.data(), rsq.data(), deepV.data(), deepBases.data(), n, nullptr));
    gx_depth_metrics_t m;
    check(S, gx_depth_metrics(&h, &m));
    fprintf(stderr, "  Depth, %s: mean %f, median %llu, %f%% of %llu bp covered\n", sampleLabel((int)h.rep, h.is_ctrl).c_str(), m.mean,
            (unsigned long long)m.median, 100.0 * m.covered_fraction, (unsigned long long)m.bases);
  }
}

// --saturation FILE [--saturation-steps N] [--saturation-seed S] [--saturation-controls]: the run's kept intervals subsampled
// on the device at N nested thresholds and the peaks called once more at each (gx_saturation), one row per point with what it
// recovers of the run's own peaks; with -v each point on stderr, the smallest fraction that recovers 90 % of the run's peaks
// and the ratio of the last two points' peak counts as the slope of the curve
void writeSaturation(State& S) {
  const Opts& o = S.o;
  gx_ctx* g = S.devs.ctx[0];
  const int N = o.saturationSteps;
  std::vector<uint64_t> thr((size_t)N);
  check(S, gx_saturation_thresholds(N, thr.data()), g);
  std::vector<gx_sat_point> pts((size_t)N);
  check(S, gx_saturation(g, thr.data(), N, o.saturationSeed, o.saturationControls ? GX_SAT_CONTROLS : 0u, pts.data()), g);   // (before the file is opened)
  writeFile(S, o.saturationFile, [&](FILE* f) { return gx_write_saturation(g, f); });
  if (!o.verbose) return;
  size_t nFull = 0;
  check(S, gx_peak_count(g, &nFull), g);
  std::vector<gx_peak> full(nFull), sub;
  if (nFull) check(S, gx_get_peaks(g, full.data(), nFull), g);
  double reach = -1.0;
  for (int j = 0; j < N; j++) {
    sub.resize((size_t)pts[j].n_peaks);
    if (!sub.empty()) check(S, gx_get_saturation_peaks(g, j, sub.data(), sub.size()), g);
    uint64_t rec = 0, in = 0, bp = 0;
    check(S, gx_saturation_overlap(full.data(), nFull, sub.data(), sub.size(), &rec, &in, &bp), g);
    const double frac = (double)thr[j] / 4294967296.0;
    fprintf(stderr, "  Saturation, %f of the intervals (%llu): %llu peaks (%llubp), %llu of the run's %zu recovered%s\n", frac,
            (unsigned long long)pts[j].n_kept, (unsigned long long)pts[j].n_peaks, (unsigned long long)pts[j].peak_bp, (unsigned long long)rec,
            nFull, pts[j].status ? " -- no analyzable fragments" : "");
    if (reach < 0 && nFull && rec * 10 >= (uint64_t)nFull * 9) reach = frac;
  }
  if (reach >= 0) fprintf(stderr, "  Saturation: %f of the intervals recover 90 %% of the run's peaks\n", reach);
  else fprintf(stderr, "  Saturation: no point recovers 90 %% of the run's peaks\n");
  if (N >= 2 && pts[N - 2].n_peaks)
    fprintf(stderr, "  Saturation: the last step added intervals by %f and peaks by %f\n", (double)thr[N - 1] / (double)thr[N - 2],
            (double)pts[N - 1].n_peaks / (double)pts[N - 2].n_peaks);
}

// --reproducibility FILE [--reproducibility-metrics FILE] [--reproducibility-overlap PCT] [--reproducibility-seed S]
// [--reproducibility-peaks PREFIX]: the peaks called once more on every replicate alone, on its two halves and on the two pools
// of halves (gx_reproducibility), one row per call in FILE and the figures made of the lists in the metrics file; with the
// prefix every call's narrowPeak and the run's own -o lines (their peak_N as in -o, so that they join with --counts) of the
// conservative and the optimal set; with -v each call on stderr, then the figures and the verdict
void writeReproducibility(State& S) {
  const Opts& o = S.o;
  gx_ctx* g = S.devs.ctx[0];
  const int nR = S.sample;
  size_t nC = 3 * (size_t)nR + 2;
  std::vector<gx_repro_call> calls(nC);
  check(S, gx_reproducibility(g, o.reproSeed, 0u, calls.data(), calls.size(), &nC), g);   // (before a file is opened)
  if (nC != calls.size()) die("", "--reproducibility: the library made other calls than this run's replicates ask for");
  writeFiles(S, o.reproFile, o.reproMetricsFile, [&](FILE* a, FILE* b) { return gx_write_reproducibility(g, o.reproPct, a, b); });
  if (!o.verbose && !o.reproPrefix) return;
  // the lists once more on this side: the sets' members and -v's lines
  size_t nRun = 0;
  check(S, gx_peak_count(g, &nRun), g);
  std::vector<gx_peak> run(nRun);
  if (nRun) check(S, gx_get_peaks(g, run.data(), nRun), g);
  std::vector<std::vector<gx_peak>> lists(nC);
  std::vector<const gx_peak*> ptrs(nC);
  for (size_t i = 0; i < nC; i++) {
    lists[i].resize((size_t)calls[i].n_peaks);
    if (!lists[i].empty()) check(S, gx_get_reproducibility_peaks(g, (int)i, lists[i].data(), lists[i].size()), g);
    ptrs[i] = lists[i].data();
  }
  gx_repro_figures fig;
  std::vector<uint64_t> pairs((size_t)nR * (nR - 1) / 2 + 1), self((size_t)nR), inRun(nC), runSup(nC);
  std::vector<uint8_t> cons(nRun + 1), opt(nRun + 1);
  check(S, gx_reproducibility_figures(run.data(), nRun, nR, calls.data(), ptrs.data(), o.reproPct, &fig, pairs.data(), self.data(), inRun.data(),
                                      runSup.data(), cons.data(), opt.data()), g);
  if (o.reproPrefix) {
    char label[64];
    for (size_t i = 0; i < nC; i++) {
      check(S, gx_reproducibility_label(&calls[i], label, sizeof label), g);
      const std::string path = std::string(o.reproPrefix) + "." + label + ".narrowPeak";
      writeFile(S, path.c_str(), [&](FILE* f) { return gx_format_narrowpeak(lists[i].data(), lists[i].size(), S.names.data(), 0, f); });
    }
    const std::pair<const char*, const std::vector<uint8_t>*> sets[2] = {{"conservative", &cons}, {"optimal", &opt}};
    for (const auto& st : sets) {
      const std::string path = std::string(o.reproPrefix) + "." + st.first + ".narrowPeak";
      writeFile(S, path.c_str(), [&](FILE* f) {
        int rc = GX_OK;
        for (size_t k = 0; k < nRun && rc == GX_OK; k++)
          if ((*st.second)[k]) rc = gx_format_narrowpeak(&run[k], 1, S.names.data(), (int)k, f);
        return rc;
      });
    }
  }
  if (!o.verbose) return;
  char label[64];
  for (size_t i = 0; i < nC; i++) {
    check(S, gx_reproducibility_label(&calls[i], label, sizeof label), g);
    fprintf(stderr, "  Reproducibility, %s: %llu intervals, %llu peaks (%llubp), %llu of them in the run's, %llu of the run's %zu supported%s\n", label,
            (unsigned long long)calls[i].n_events, (unsigned long long)calls[i].n_peaks, (unsigned long long)calls[i].peak_bp,
            (unsigned long long)inRun[i], (unsigned long long)runSup[i], nRun, calls[i].status ? " -- no analyzable fragments" : "");
  }
  static const char* const verdict[] = {"pass", "borderline", "fail", "NA"};
  if (nR > 1)
    fprintf(stderr, "  Reproducibility: Nt %llu (t%d, t%d), Np %llu, N_self %llu .. %llu\n", (unsigned long long)fig.nt, fig.best_i + 1, fig.best_j + 1,
            (unsigned long long)fig.np, (unsigned long long)fig.n_self_min, (unsigned long long)fig.n_self_max);
  else
    fprintf(stderr, "  Reproducibility: one replicate: Np %llu, N_self %llu\n", (unsigned long long)fig.np, (unsigned long long)fig.n_self_max);
  if (fig.verdict == GX_REPRO_NA)
    fprintf(stderr, "  Reproducibility: verdict NA (%s)\n", nR > 1 ? "a count of 0" : "the ratios need two replicates");
  else
    fprintf(stderr, "  Reproducibility: rescue ratio %f, self-consistency ratio %f: verdict %s\n", fig.rescue, fig.self_consistency, verdict[fig.verdict]);
  fprintf(stderr, "  Reproducibility: conservative set %llu peaks, optimal set %llu peaks\n", (unsigned long long)fig.n_conservative,
          (unsigned long long)fig.n_optimal);
}

// --profile BED --profile-out PREFIX: each sample's pileup summed over bins around the BED's anchor sites.  The anchors go to
// every context before the first sample (setProfile); PREFIX.profile.tsv has the mean signal per base and anchor at every
// offset, one column per sample; with --profile-matrix a sample's PREFIX.t<rep>.matrix.tsv / PREFIX.c<rep>.matrix.tsv has one
// row per BED line, in the BED's order; with -v the enrichment of each sample
ProfilePlan planProfile(State& S) {
  ProfilePlan P;
  P.names = ChromNames(S.chrom);
  const size_t n = S.anchorRows.size();
  P.anchors.resize(n);
  P.regions.resize(n);
  P.rowNames.resize(n);
  for (size_t k = 0; k < n; k++) {
    const RegionRow& r = S.anchorRows[k];
    const uint32_t ci = P.names.of(r.chrom);   // (an index behind the table: the library's row is zero)
    const int strand = S.anchorStrand[k];
    const uint32_t pos = S.o.profileCenter ? (uint32_t)(((uint64_t)r.start + r.end) / 2) : strand > 0 ? r.start : r.end - 1;
    P.anchors[k] = gx_anchor{ci, pos, strand};
    P.regions[k] = gx_region{ci, r.start, r.end};
    P.rowNames[k] = r.named ? r.name.c_str() : nullptr;
    if (ci < S.chrom.size() && !S.chrom[ci].skip && S.chrom[ci].len != 0) P.counted++;
  }
  return P;
}
void writeProfile(State& S) {
  const Opts& o = S.o;
  const ProfilePlan& P = S.profilePlan;
  const int nS = (int)S.sampleNames.size();
  agreedSamples(S, "--profile: the library closed another number of samples than were read", gx_profile_samples, nS);
  writeFile(S, (std::string(o.profilePrefix) + ".profile.tsv").c_str(), [&](FILE* f) {
    return gx_write_profile_group(S.devs.ctx.data(), (int)S.devs.n(), nS, S.sampleNames.data(), P.counted, f);
  });
  const uint32_t nb = (uint32_t)(2 * o.flank / o.profileBin);
  const ClosedSamples L = closedSamples(S, true);
  std::vector<int64_t> agg(nb), one(nb);
  for (int i = 0; i < nS; i++) {
    std::fill(agg.begin(), agg.end(), 0);
    for (gx_ctx* g : S.devs.ctx) {
      check(S, gx_get_profile(g, i, nullptr, nullptr, one.data(), nullptr, 0, 0), g);
      for (uint32_t j = 0; j < nb; j++) agg[j] += one[j];
    }
    if (o.profileMatrix)
      writeFile(S, (std::string(o.profilePrefix) + "." + L.labels[i] + ".matrix.tsv").c_str(), [&](FILE* f) {
        return gx_write_profile_rows_group(S.devs.ctx.data(), (int)S.devs.n(), i, P.names.all.data(), P.regions.data(), P.rowNames.data(),
                                           P.anchors.data(), f);
      });
    if (!o.verbose) continue;
    // the highest bin over the mean of the first and the last ne bins (100 bases at each end, at least one bin, at most a
    // quarter of the bins): with the defaults ENCODE's TSS-enrichment construction, unsmoothed
    const uint32_t ne = std::max(1u, std::min(nb / 4, (uint32_t)((100 + o.profileBin - 1) / o.profileBin)));
    __int128 edge = 0;
    int64_t top = agg[0];
    for (uint32_t j = 0; j < nb; j++) {
      top = std::max(top, agg[j]);
      if (j < ne || j >= nb - ne) edge += agg[j];
    }
    fprintf(stderr, "  Profile, %s: enrichment %f over %zu anchors\n", sampleLabel(L.reps[i], L.ctrls[i]).c_str(),
            edge ? (double)top * (2.0 * ne) / (double)edge : 0.0, P.counted);
  }
}

// ---- the table of figures ---------------------------------------------------------------------------------------------------
// One row per figure, in the order they are written: when it is on, what it is made of besides the pileups, and its writer
enum : unsigned { KEPT = 1, BINS = 2 };   // the library keeps the samples' intervals (gx_set_count_in_peaks); the coverage bins
struct Figure { bool (*on)(const Opts&); unsigned madeOf; void (*write)(State&); };
const Figure FIGURES[] = {
    {[](const Opts& o) { return o.countsFile != nullptr; }, KEPT, writeCounts},
    {[](const Opts& o) { return o.peakSignalFile != nullptr; }, KEPT, writePeakSignal},
    {[](const Opts& o) { return o.summitsFile != nullptr; }, KEPT, writeSummits},
    {[](const Opts& o) { return o.regionsBed != nullptr; }, KEPT, writeRegionCounts},
    {[](const Opts& o) { return o.coveragePrefix != nullptr; }, BINS, writeCoverage},
    {[](const Opts& o) { return o.correlationFile != nullptr; }, BINS, writeCorrelation},
    {[](const Opts& o) { return o.spearmanFile != nullptr; }, BINS, writeSpearman},
    {[](const Opts& o) { return o.fingerprintFile != nullptr; }, BINS, writeFingerprint},
    {[](const Opts& o) { return o.complexityFile != nullptr; }, KEPT, writeComplexity},
    {[](const Opts& o) { return o.lengthsOn(); }, KEPT, writeIntervalStats},
    {[](const Opts& o) { return o.depthOn(); }, 0, writeDepth},
    {[](const Opts& o) { return o.xcorOn(); }, 0, writeXcor},
    {[](const Opts& o) { return o.gcBiasFile != nullptr; }, KEPT, writeGcBias},
    {[](const Opts& o) { return o.gcPeaksFile != nullptr; }, 0, writeGcPeaks},
    {[](const Opts& o) { return o.motifsFile != nullptr; }, 0, writeMotifs},
    {[](const Opts& o) { return o.kmersFile != nullptr; }, 0, writeKmers},
    {[](const Opts& o) { return o.saturationFile != nullptr; }, KEPT, writeSaturation},
    {[](const Opts& o) { return o.reproOn(); }, KEPT, writeReproducibility},
    {[](const Opts& o) { return o.profileBed != nullptr; }, 0, writeProfile},
};
bool someFigureOf(const Opts& o, unsigned what) {
  return std::any_of(std::begin(FIGURES), std::end(FIGURES), [&](const Figure& f) { return (f.madeOf & what) && f.on(o); });
}
bool keepsIntervals(const Opts& o) { return someFigureOf(o, KEPT); }
bool Opts::binsOn() const { return someFigureOf(*this, BINS); }

}  // namespace
