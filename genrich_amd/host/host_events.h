// host_events.h -- from the alignments of one read name to events: where results go (Sink), saveInterval, fragments and unpaired
// alignments, multimap weighting, processAlns.  (a part of genrich_amd.cpp's translation unit)
#pragma once
namespace {

// ---- where a read-name group's results go -----------------------------------------------------
// Read-name groups do not depend on each other, only their results have an order: the events (the int16 replay of
// the library goes by it), the -b lines, the -v warnings (and the count that suppresses them after the first 128),
// the additions into the float sum behind the -x average.  A worker thread that takes a chunk of whole groups
// (parallel state, below) has `t_sink` set: everything that would touch the run's state is written there instead and
// merged into the state by its owner, chunk after chunk in file order.  Without a sink (one thread; the tails of
// finishFile) the state is written directly, as before.
struct Sink {
  std::vector<gx_event> ev;
  std::string bed;                                      // -b lines
  std::vector<std::pair<std::string, bool>> warn;       // stderr lines in order; true: counts towards errCount
  std::vector<double> lenTerms;                         // C.totalLen += ... in order (a float sum: not associative)
  std::vector<gx_tag> tags;                             // --xcor: strand-tagged 5' ends (any order)
  bool unpairedTags = false;
};
thread_local Sink* t_sink = nullptr;

std::string vformat(const char* fmt, va_list ap) {
  va_list ap2;
  va_copy(ap2, ap);
  const int n = vsnprintf(nullptr, 0, fmt, ap2);
  va_end(ap2);
  std::string out((size_t)std::max(0, n), '\0');
  if (n > 0) vsnprintf(&out[0], (size_t)n + 1, fmt, ap);
  return out;
}
// a warning that takes part in the "(another N warning messages suppressed)" count (saveInterval's two)
void warnCounted(State& S, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (t_sink)
    t_sink->warn.emplace_back(vformat(fmt, ap), true);
  else {
    if (S.errCount < MAX_ALNS) vfprintf(stderr, fmt, ap);
    S.errCount++;
  }
  va_end(ap);
}
// ... and one that does not
void warnPlain(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (t_sink) t_sink->warn.emplace_back(vformat(fmt, ap), false);
  else vfprintf(stderr, fmt, ap);
  va_end(ap);
}
void pushEvent(State& S, const gx_event& e) {  // (state's side: the library takes the events in pieces of 2^20)
  if (!S.gx && S.hot.on) S.hot.all.push_back(e);
  S.buf.push_back(e);
  if (S.buf.size() >= (1u << 20)) {
    if (S.gx && S.sampleOpen) flushEvents(S);
    if (!S.gx || S.sampleOpen) S.buf.clear();  // (--events-only: nothing to send them to; with -b the int16 decisions keep their own copy, hot.all)
  }
}

// --xcor: the 5' end of an alignment that becomes intervals, from its own coordinates (before -j / -y / -w / -x and
// saveInterval's clamping change them, and whether or not the int16 replay drops the interval)
void saveTag(State& S, int ci, bool plus, uint32_t pos, bool unpaired) {
  const gx_tag t{(uint32_t)ci, pos, plus ? 1u : 0u};
  if (t_sink) {
    t_sink->tags.push_back(t);
    t_sink->unpairedTags |= unpaired;
    return;
  }
  S.tags.push_back(t);
  S.unpairedTags |= unpaired;
  if (S.tags.size() >= (1u << 20) && S.sampleOpen) flushTags(S);
}
// an unpaired alignment: forward (+, first base), reverse (-, last base; pos[1] is the exclusive end)
void saveUnpairTag(State& S, int ci, const uint32_t* pos, bool strand) {
  if (S.o.xcorOn()) saveTag(S, ci, strand, strand ? pos[0] : pos[1] - 1u, true);
}

// A loaded window's exact difference (1/120 units per base): from the device, which is sent what the host still holds first.
std::vector<long long>& hotLoad(State& S, uint32_t ci, size_t gw) {
  auto it = S.hot.win.find(gw);
  if (it != S.hot.win.end()) return it->second;
  if (S.gx && S.sampleOpen && !S.buf.empty()) {
    flushEvents(S);
    S.buf.clear();
  }
  std::vector<long long> net((size_t)1 << HotWindows::WB, 0);
  const uint32_t pos0 = (uint32_t)((gw - S.hot.base[ci]) << HotWindows::WB);
  const uint32_t n = std::min<uint32_t>(1u << HotWindows::WB, S.chrom[ci].len + 1 - pos0);
  if (!S.gx) {  // --events-only: no device to ask; the sample's events were kept for this
    for (const gx_event& e : S.hot.all) {
      if (e.chrom != ci) continue;
      const long long w = gxsat::weight_of(e.count);
      if (e.start - pos0 < n) net[e.start - pos0] += w;
      if (e.end - pos0 < n) net[e.end - pos0] -= w;
    }
  } else if (S.sampleOpen) {
    gx_ctx* g = S.devs.n() == 1 ? S.gx : S.devs.ctx[S.devs.owner[ci]];
    check(S, gx_window_net(g, ci, pos0, n, net.data()), g);
  }
  return S.hot.win.emplace(gw, std::move(net)).first->second;
}
// the state's owner, one event at a time: false when the reference would have dropped it (its warning printed)
bool hotKeeps(State& S, const gx_event& e, const char* qname) {
  HotWindows& H = S.hot;
  const long long w = gxsat::weight_of(e.count);
  if (!w) return true;  // (the library reports the count: ERRALNS)
  const size_t a = H.base[e.chrom] + (e.start >> HotWindows::WB), b = H.base[e.chrom] + (e.end >> HotWindows::WB);
  const bool nearA = H.ws[a] + (uint32_t)w >= (uint32_t)gxsat::HOT, nearB = H.we[b] + (uint32_t)w >= (uint32_t)gxsat::HOT;
  if (nearA || nearB || !H.win.empty()) {
    std::vector<long long>* wa = nearA || H.win.count(a) ? &hotLoad(S, e.chrom, a) : nullptr;
    std::vector<long long>* wb = nearB || H.win.count(b) ? &hotLoad(S, e.chrom, b) : nullptr;
    const Chrom& c = S.chrom[e.chrom];
    if (wa && gxsat::canon_cov((*wa)[e.start & HotWindows::WMASK]) == 32767) {
      if (S.o.verbose) {
        fprintf(stderr, "Warning! Read %s, alignment at (%s, %ld-%ld)", qname, c.name.c_str(), (long)e.start, (long)e.end);
        fprintf(stderr, " skipped due to overflow\n");
      }
      return false;
    }
    if (wb && gxsat::canon_cov((*wb)[e.end & HotWindows::WMASK]) == -32768) {
      if (S.o.verbose) {
        fprintf(stderr, "Warning! Read %s, alignment at (%s, %ld-%ld)", qname, c.name.c_str(), (long)e.start, (long)e.end);
        fprintf(stderr, " skipped due to underflow\n");
      }
      return false;
    }
    if (wa) (*wa)[e.start & HotWindows::WMASK] += w;
    if (wb) (*wb)[e.end & HotWindows::WMASK] -= w;
  }
  H.ws[a] += (uint32_t)w;
  H.we[b] += (uint32_t)w;
  return true;
}

// ---- saveInterval (2516-2591): clamp, event, -b line ----------------------------------------
uint32_t saveInterval(State& S, int ci, int64_t start, int64_t end, const char* qname, uint8_t count) {
  Chrom& c = S.chrom[ci];
  if (start < 0) {
    if (S.o.verbose) warnCounted(S, "Warning! Read %s prevented from extending below 0 on %s\n", qname, c.name.c_str());
    start = 0;
  }
  if (start >= c.len) {
    std::string msg = std::string("Read ") + qname + ", ref. " + c.name;
    if (msg.size() > 511) msg.resize(511);  // (snprintf into char msg[512])
    die(msg, ": read aligned beyond reference end");
  }
  if (end > c.len) {
    if (S.o.verbose) warnCounted(S, "Warning! Read %s prevented from extending past %d on %s\n", qname, c.len, c.name.c_str());
    end = c.len;
  }
  const gx_event e{(uint32_t)ci, (uint32_t)start, (uint32_t)end, count};
  if (t_sink) t_sink->ev.push_back(e);
  else {
    if (S.hot.on && !hotKeeps(S, e, qname)) return 0;  // 2558-2573
    pushEvent(S, e);
  }
  if (S.bedOpt) {
    if (t_sink) {
      char num[96];
      std::string& b = t_sink->bed;
      b += c.name;
      snprintf(num, sizeof num, "\t%ld\t%ld\t", (long)start, (long)end);
      b += num;
      b += qname;
      snprintf(num, sizeof num, "_%d_%c_%d\n", count, S.ctrl ? 'C' : 'E', S.sample);
      b += num;
    } else
      fprintf(S.bed.f, "%s\t%ld\t%ld\t%s_%d_%c_%d\n", c.name.c_str(), (long)start, (long)end, qname, count,
              S.ctrl ? 'C' : 'E', S.sample);
  }
  return (uint32_t)(end - start);
}

// ---- alignments of one read name -------------------------------------------------------------
struct Aln {
  uint32_t pos[2];
  float score;
  bool primary, paired, full, first, strand;
  int chrom;
};
struct Unpair { int chrom; uint32_t pos[2]; bool strand; uint8_t count; std::string name; };

struct Counts {
  uint64_t count = 0, unmapped = 0, paired = 0, single = 0, orphan = 0, pairedPr = 0, singlePr = 0, supp = 0,
           skipped = 0, lowMapQ = 0, secPair = 0, secSingle = 0;
  uint64_t countPr = 0, dupsPr = 0, countDc = 0, dupsDc = 0, countSn = 0, dupsSn = 0;  // -r
  double totalLen = 0.0;
};

// (positions are uint32_t in the reference and its sums with the extension / ATAC lengths wrap in 32 bits
// before they reach saveInterval's int64_t parameters; a position can be "negative" -- wrapped -- when the
// BAM reader made it from a record without SEQ)
uint32_t saveFragment(State& S, const char* qname, const Aln& a, uint8_t count) {  // 2754-2774, 2728-2749
  uint32_t start = a.pos[0], end = a.pos[1];
  if (start > end) std::swap(start, end);
  if (S.o.xcorOn() && !S.o.xcorUnpaired) {   // a proper pair: (+, its first base) and (-, its last base)
    saveTag(S, a.chrom, true, start, false);
    saveTag(S, a.chrom, false, end - 1u, false);
  }
  if (!S.o.atacOpt) return saveInterval(S, a.chrom, start, end, qname, count);
  if (S.o.atacAdj) { start += 5; end += (uint32_t)-5; }
  if (start + S.o.atacLen3 >= (uint32_t)(int)(end - S.o.atacLen3))
    return saveInterval(S, a.chrom, (int)(start - S.o.atacLen5), (uint32_t)(end + S.o.atacLen5), qname, count);
  return saveInterval(S, a.chrom, (int)(start - S.o.atacLen5), (uint32_t)(start + S.o.atacLen3), qname, count) +
         saveInterval(S, a.chrom, (int)(end - S.o.atacLen3), (uint32_t)(end + S.o.atacLen5), qname, count);
}

void saveUnpair(State& S, const char* qname, Aln& a, uint8_t count) {  // 2689-2721
  const Opts& o = S.o;
  saveUnpairTag(S, a.chrom, a.pos, a.strand);
  if (o.extendOpt) {
    if (a.strand) saveInterval(S, a.chrom, a.pos[0], (uint32_t)(a.pos[0] + o.extend), qname, count);
    else saveInterval(S, a.chrom, (int)(a.pos[1] - o.extend), a.pos[1], qname, count);
  } else if (o.atacOpt) {
    if (a.strand) {
      if (o.atacAdj) a.pos[0] += 5;
      saveInterval(S, a.chrom, (int)(a.pos[0] - o.atacLen5), (uint32_t)(a.pos[0] + o.atacLen3), qname, count);
    } else {
      if (o.atacAdj) a.pos[1] += (uint32_t)-5;
      saveInterval(S, a.chrom, (int)(a.pos[1] - o.atacLen3), (uint32_t)(a.pos[1] + o.atacLen5), qname, count);
    }
  } else
    saveInterval(S, a.chrom, a.pos[0], a.pos[1], qname, count);
}

bool usable(const State& S, const Aln& a) { return S.chrom[a.chrom].save && !S.chrom[a.chrom].skip; }

// new minimum score so that the number of kept alignments is one of 1,2,3,4,5,6,8,10 (2985, 3089)
void subsample(const std::vector<float>& scoresDesc, uint8_t& count, float& score) {
  count = count > 10 ? 10 : count - 1;
  score = scoresDesc[count - 1];
}

int processPair(State& S, const char* qname, std::vector<Aln>& aln, Counts& C, float score) {  // 3122-3176
  if (score != NOSCORE) score -= S.o.asDiff;
  auto ok = [&](const Aln& a) { return a.paired && a.full && a.score >= score && usable(S, a); };
  uint8_t count = 0;
  for (auto& a : aln) count += ok(a);
  if (!count) return 0;
  if (count > 10 || count == 7 || count == 9) {
    std::vector<float> sc;
    for (auto& a : aln)
      if (ok(a)) {  // stable insertion, descending
        size_t j = 0;
        while (j < sc.size() && !(a.score > sc[j])) j++;
        sc.insert(sc.begin() + j, a.score);
      }
    subsample(sc, count, score);
  }
  uint64_t fragLen = 0;
  uint8_t saved = 0;
  for (auto& a : aln)
    if (ok(a)) {
      fragLen += saveFragment(S, qname, a, count);
      if (++saved == count) break;  // in case of AS ties
    }
  if (t_sink) t_sink->lenTerms.push_back((double)fragLen / count);  // (added by the state's owner, in file order)
  else C.totalLen += (double)fragLen / count;
  return 1;
}

int processSingle(State& S, const char* qname, std::vector<Aln>& aln, std::vector<Unpair>& unpair, float score,
                  bool first) {  // 3019-3083
  if (score != NOSCORE) score -= S.o.asDiff;
  auto ok = [&](const Aln& a) { return !a.paired && a.first == first && a.score >= score && usable(S, a); };
  uint8_t count = 0;
  for (auto& a : aln) count += ok(a);
  if (!count) return 0;
  if (count > 10 || count == 7 || count == 9) {
    std::vector<float> sc;
    for (auto& a : aln)
      if (ok(a)) {
        size_t j = 0;
        while (j < sc.size() && !(a.score > sc[j])) j++;
        sc.insert(sc.begin() + j, a.score);
      }
    subsample(sc, count, score);
  }
  uint8_t saved = 0;
  for (auto& a : aln)
    if (ok(a)) {
      if (S.o.avgExtOpt)
        unpair.push_back(Unpair{a.chrom, {a.pos[0], a.pos[1]}, a.strand, count, qname});
      else
        saveUnpair(S, qname, a, count);
      if (++saved == count) break;
    }
  return 1;
}

// -r keeps the sets instead (host_dups.h, which replays them through processPair / processSingle above)
struct DupReads;
void saveAlns(const State& S, const char* qname, const std::vector<Aln>& aln, bool pair, bool singleR1, bool singleR2,
              float scorePr, float scoreR1, float scoreR2, uint16_t qualR1, uint16_t qualR2, DupReads& D);

void processAlns(State& S, const char* qname, std::vector<Aln>& aln, std::vector<Unpair>& unpair, Counts& C,
                 uint16_t qualR1, uint16_t qualR2, DupReads& D) {  // 3187-3265
  float scorePr = NOSCORE, scoreR1 = NOSCORE, scoreR2 = NOSCORE;
  bool pair = false, singleR1 = false, singleR2 = false;
  for (auto& a : aln) {
    if (a.paired) {
      if (a.full) {
        if (!pair || scorePr < a.score) scorePr = a.score;
        pair = true;
      } else
        C.orphan++;
    } else if (S.o.singleOpt && !pair) {
      if (a.first && scoreR1 <= a.score) { scoreR1 = a.score; singleR1 = true; }
      else if (!a.first && scoreR2 <= a.score) { scoreR2 = a.score; singleR2 = true; }
    }
  }
  if (S.o.dupsOpt)
    saveAlns(S, qname, aln, pair, singleR1, singleR2, scorePr, scoreR1, scoreR2, qualR1, qualR2, D);
  else if (pair)
    C.pairedPr += processPair(S, qname, aln, C, scorePr);
  else if (S.o.singleOpt) {
    if (singleR1) C.singlePr += processSingle(S, qname, aln, unpair, scoreR1, true);
    if (singleR2) C.singlePr += processSingle(S, qname, aln, unpair, scoreR2, false);
  }
}

}  // namespace
