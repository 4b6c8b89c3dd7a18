// host_ingest.h -- SAM and BAM decoding and the threads it runs on: parseAlign, the decode pipeline, the parallel state workers,
// readSAM / readBAM, the -v accounting and the header pre-scan.  (a part of genrich_amd.cpp's translation unit)
#pragma once
namespace {

// parseAlign (4141-4212); returns false when the per-read alignment limit is hit
bool parseAlign(State& S, std::vector<Aln>& aln, uint16_t flag, int ci, uint32_t pos, int length, uint32_t pnext,
                Counts& C, float score) {
  if (flag & 0x1) {
    if ((flag & 0xC0) == 0xC0) die("", "Linear template with >2 reads -- not allowed");
    if (!(flag & 0xC0)) die("", "Unknown index of paired alignment");
  }
  const Chrom& ch = S.chrom[ci];
  const uint32_t end5 = (flag & 0x10) ? pos + length : pos;  // 5' end of a reverse read = pos + refLen
  if ((flag & 0x3) == 0x3) {
    if (ch.skip || !ch.save) C.skipped++;
    else {
      C.paired++;
      if (flag & 0x100) C.secPair++;
    }
    for (auto& a : aln)
      if (a.paired && !a.full && a.chrom == ci &&
          ((flag & 0x40) ? (!a.first && a.pos[0] == pos) : (a.first && a.pos[1] == pos)) &&
          ((flag & 0x100) ? !a.primary : a.primary)) {
        if (flag & 0x40) a.pos[0] = end5; else a.pos[1] = end5;  // updatePairedAln 4049
        if (score == NOSCORE) a.score = NOSCORE;
        else if (a.score != NOSCORE) a.score += score;
        a.full = true;
        return true;
      }
    if (aln.size() == MAX_ALNS) return false;
    Aln a{};
    a.chrom = ci;
    a.score = score;
    a.primary = !(flag & 0x100);
    a.full = false;
    a.paired = true;
    if (flag & 0x40) { a.pos[0] = end5; a.pos[1] = pnext; a.first = true; }
    else { a.pos[0] = pnext; a.pos[1] = end5; a.first = false; }
    aln.push_back(a);
    return true;
  }
  if (ch.skip || !ch.save) C.skipped++;
  else {
    C.single++;
    if (flag & 0x100) C.secSingle++;
  }
  if (S.o.singleOpt) {
    if (aln.size() == MAX_ALNS) return false;
    Aln a{};
    a.chrom = ci;
    a.score = score;
    a.primary = !(flag & 0x100);
    a.paired = false;
    a.strand = !(flag & 0x10);
    a.first = flag & 0x40;
    a.pos[0] = pos;
    a.pos[1] = pos + length;
    aln.push_back(a);
  }
  return true;
}

// distance to the 3' end from a SAM CIGAR (parseCigar 4408, calcDist 4451)
int calcDist(const char* qname, const char* seq, const char* cigar) {
  int length = strcmp(seq, "*") ? (int)strlen(seq) : 0;
  int offset = 0;
  if (strcmp(cigar, "*")) {
    int len = 0;
    const char* p = cigar;
    while (*p) {
      char* e;
      long n = strtol(p, &e, 10);
      if (e == p && (*p < '0' || *p > '9')) n = 0;  // an op without a number counts as 0
      char op = *e;
      if (!op) break;
      switch (op) {
        case 'M': case '=': case 'X': len += (int)n; break;
        case 'I': case 'S': len += (int)n; offset -= (int)n; break;
        case 'D': offset += (int)n; break;
        case 'N': case 'H': case 'P': break;
        default: {
          char msg[4] = "' '";
          msg[1] = op;
          die(msg, ": unknown Op in CIGAR");
        }
      }
      p = e + 1;
    }
    if (!length) length = len;
    else if (length != len) die(qname, ": mismatch between sequence length and CIGAR");
  } else if (!length)
    die(qname, ": no sequence information (SEQ or CIGAR)");
  return length + offset;
}

float samScore(char* extra) {  // getScore 4383-4402
  // fields on TAB; inside a field the tokens between colons (strtok: a run of colons is one separator).
  // The first field whose first token is "AS" decides: its third token is the score, whatever the second
  // (the type) says; without a third token there is no score.
  if (!extra) return NOSCORE;
  char* endF = nullptr;
  for (char* f = strtok_r(extra, "\t", &endF); f; f = strtok_r(nullptr, "\t", &endF)) {
    char* endT = nullptr;
    char* tag = strtok_r(f, ":", &endT);
    if (tag && !strcmp(tag, "AS")) {
      if (!strtok_r(nullptr, ":", &endT)) return NOSCORE;
      char* v = strtok_r(nullptr, ":", &endT);
      return v ? getFloat(v) : NOSCORE;
    }
  }
  return NOSCORE;
}

void headerLine(State& S, char* line) {  // checkHeader 4307-4342, loadChrom 4275-4299
  // as the reference cuts it up: strtok on TAB, so the last token of the line still carries its '\n' -- a
  // bare "@HD\n" or "@SQ\n" is therefore not recognised -- and only the values of SO: / SN: / LN: are cut at
  // the line feed (a carriage return stays)
  auto cut = [](char* v) {
    if (v) v[strcspn(v, "\n")] = '\0';
  };
  char* tag = strtok(line, "\t");
  if (!tag) return;
  if (!strcmp(tag, "@HD")) {
    char* order = nullptr;
    for (char* f = strtok(nullptr, "\t"); f; f = strtok(nullptr, "\t"))
      if (!strncmp(f, "SO:", 3)) order = f + 3;
    cut(order);
    if (S.o.sortOpt && (!order || strcmp(order, "queryname")))
      die("", "SAM/BAM file not sorted by queryname (samtools sort -n)");
  } else if (!strcmp(tag, "@SQ")) {
    char *name = nullptr, *len = nullptr;
    for (char* f = strtok(nullptr, "\t"); f; f = strtok(nullptr, "\t")) {
      if (!strncmp(f, "SN:", 3)) name = f + 3;
      else if (!strncmp(f, "LN:", 3)) len = f + 3;
    }
    if (!name || !len) return;
    cut(name);
    cut(len);
    saveChrom(S, name, (uint32_t)getInt(len));
  }
}

// the header of the current file is complete: open the sample on the device
void openSample(State& S) {
  if (S.sampleOpen) return;
  S.sampleOpen = true;
  if (!S.gx) {
    if (S.hot.on) S.hot.init(S.chrom);
    return;
  }
  std::vector<uint8_t> save(S.chrom.size());
  for (size_t k = 0; k < S.chrom.size(); k++) save[k] = S.chrom[k].save;
  for (gx_ctx* g : S.devs.ctx) check(S, gx_sample_begin(g, S.ctrl ? 1 : 0, S.ctrl ? nullptr : save.data()), g);
  if (S.hot.on) S.hot.init(S.chrom);  // (the reference's difference arrays start at zero with every file)
}

struct ReadSet {
  std::string name;
  std::vector<Aln> aln;
  std::vector<Unpair> unpair;
  bool have = false;
  uint16_t qualR1 = 0, qualR2 = 0;  // -r: base-quality sums of the two mates of the current read
  DupReads dup;                     // -r: every alignment set of the file
};

void flushSet(State& S, ReadSet& rs, Counts& C) {
  if (rs.have) processAlns(S, rs.name.c_str(), rs.aln, rs.unpair, C, rs.qualR1, rs.qualR2, rs.dup);
  rs.aln.clear();
  rs.qualR1 = rs.qualR2 = 0;
}

// sumQual 4127-4134, bug for bug: `qual[0] == 0xFF` compares a (signed) char with 255 and never
// holds, so a BAM record without qualities (all 0xFF = -1) sums to -len and wraps
uint16_t sumQual(const char* qual, int len, int offset) {
  int sum = 0;
  for (int i = 0; i < len; i++) sum += (int)(signed char)qual[i] - offset;
  return sum > UINT16_MAX ? UINT16_MAX : (uint16_t)sum;
}

// one alignment record, format independent (the tail of readSAM's / parseBAM's loop)
void record(State& S, ReadSet& rs, Counts& C, const char* qname, uint16_t flag, int ci, uint32_t pos, uint8_t mapq,
            int length, uint32_t pnext, float score, const char* qual, int qualLen, int qualOffset) {
  if (mapq < S.o.minMapQ) { C.lowMapQ++; return; }
  if (!t_sink) openSample(S);  // the header is complete once the first record arrives (workers: the state's owner does it)
  if (!rs.have || rs.name != qname) {
    flushSet(S, rs, C);
    rs.have = true;
    rs.name.assign(qname, strnlen(qname, MAX_ALNS));  // strncpy(readName, qname, MAX_ALNS)
  }
  if (S.o.dupsOpt && !(((flag & 0x1) && ((flag & 0xC0) == 0xC0 || !(flag & 0xC0))))) {  // parseAlign 4155-4164
    uint16_t& q = (flag & 0x40) ? rs.qualR1 : rs.qualR2;
    const bool star = qualLen >= 1 && qual[0] == '*' && (qualLen == 1 || qual[1] == '\0');  // strcmp(qual, "*")
    if (!q && !star) q = sumQual(qual, qualLen, qualOffset);
  }
  if (!parseAlign(S, rs.aln, flag, ci, pos, length, pnext, C, score) && S.o.verbose)
    warnPlain("Warning! Read %s has more than %d alignments\n", qname, MAX_ALNS);
}

void finishFile(State& S, ReadSet& rs, Counts& C) {  // the tail of readSAM / parseBAM
  flushSet(S, rs, C);
  if (S.o.dupsOpt) {
    findDups(S, rs.dup, C);
    return;
  }
  if (S.o.avgExtOpt) {  // processAvgExt 2614-2647
    int avgLen = 0;
    if (!C.pairedPr) {
      if (S.o.verbose) {
        fprintf(stderr, "Warning! No paired alignments to calculate avg frag ");
        fprintf(stderr, "length --\n  Printing unpaired alignments \"as is\"\n");
      }
    } else
      avgLen = (int)(C.totalLen / C.pairedPr + 0.5);
    for (auto& u : rs.unpair) {
      saveUnpairTag(S, u.chrom, u.pos, u.strand);
      if (!avgLen) saveInterval(S, u.chrom, u.pos[0], u.pos[1], u.name.c_str(), u.count);
      else if (u.strand) saveInterval(S, u.chrom, u.pos[0], (uint32_t)(u.pos[0] + avgLen), u.name.c_str(), u.count);
      else saveInterval(S, u.chrom, (int)(u.pos[1] - avgLen), u.pos[1], u.name.c_str(), u.count);
    }
    rs.unpair.clear();
  }
}

// ---- record decoding, apart from the run's state ---------------------------------------------
// What readSAM's / readBAM's loop knows about a record BEFORE it touches the run's state -- the fields cut up and
// converted, the reference sequence looked up, the distance to the 3' end, the alignment score -- depends on nothing
// but the record (and the header, which is complete by then).  That part, three quarters of the parsing thread's
// time on bowtie2-style SAM text, runs on `--threads` decoder threads over batches of records; the rest -- counters,
// read-name groups, pairing, weights, -b lines, events: everything whose order matters -- stays on the one thread
// that owns the state and takes the decoded batches in file order.  An error found while decoding is kept with its
// record and raised when its turn comes, so warnings and errors appear in the order of a sequential run.
struct Decoded {
  enum Kind : uint8_t { REC, UNMAPPED, SUPP, LOWQ, FAIL };
  uint8_t kind = REC, mapq = 0;
  uint16_t flag = 0;
  int ci = 0, length = 0, qualLen = 0;
  uint32_t pos = 0, pnext = 0;
  float score = 0.0f;
  uint32_t qname = 0, qual = 0;   // offsets from the record's first byte
  int fail = -1;                   // FAIL: index into the batch's messages
};

constexpr size_t REC_MAX = 65520;  // (a line is read in pieces of at most 65,520 bytes: readSAM's buffer)
// bytes of records per batch (GENRICH_BATCH_BYTES: tests cut the input into batches of a line or two)
const size_t BATCH_BYTES = getenv("GENRICH_BATCH_BYTES") ? (size_t)std::max(1L, atol(getenv("GENRICH_BATCH_BYTES"))) : (size_t)1 << 20;

struct Batch {
  std::unique_ptr<char[]> bytes;   // the records' text lines (NUL-terminated) or BAM blocks
  size_t used = 0, cap = 0;
  std::vector<uint32_t> off, len;  // one entry per record
  std::vector<Decoded> rec;
  std::vector<std::pair<std::string, std::string>> fails;
  // What the thread that cuts the stream into chunks needs to know about a record, one byte each (made by the decoder
  // that has the records in its cache: the cutting thread reads 64 records per cache line instead of two lines per
  // record): [2:0] the record's kind, MARK_SAME when it has the name of the group the REC record before it IN THIS
  // BATCH belongs to (record()'s comparison with its 128-character quirk); the first REC record of a batch is compared
  // by the cutting thread itself, with the name it carries over (lastName: this batch's contribution to that)
  static constexpr uint8_t MARK_SAME = 0x80;
  std::vector<uint8_t> mark;
  uint32_t firstRec = 0xFFFFFFFFu;  // index of the batch's first REC record
  std::string lastName;             // the name of the group the batch's last REC record belongs to, as record() keeps it
  bool decoded = false;
  // a batch of text that the READER only delimited (a span of a mapped file that ends behind a line feed): the
  // decoder that takes the batch cuts it into lines itself (cutSpan) -- the reader's part is then a memchr per batch
  const char* span = nullptr;
  size_t spanLen = 0;
  // records that stay where they are -- BAM blocks inside an inflated BGZF member, which `holds` keeps alive: off[i] has
  // its top bit set and indexes `ext`
  std::vector<const char*> ext;
  std::vector<std::shared_ptr<const void>> holds;
  size_t extBytes = 0;
  static constexpr uint32_t EXT = 0x80000000u;
  const char* at(size_t i) const { return (off[i] & EXT) ? ext[off[i] & ~EXT] : bytes.get() + off[i]; }
  void addExt(const void* p, size_t n) {
    off.push_back(EXT | (uint32_t)ext.size());
    len.push_back((uint32_t)n);
    ext.push_back(static_cast<const char*>(p));
    extBytes += n;
  }
  bool hasWork() const { return !off.empty() || spanLen; }
  void reset(size_t want) {  // (the reader's thread, before the batch is queued)
    decoded = false;
    clearRecords(want);
  }
  // ... and what a decoder may do to a queued batch: `decoded` belongs to the pipe's mutex (the taker polls it)
  void clearRecords(size_t want) {
    if (cap < want) {
      bytes.reset(new char[want]);
      cap = want;
    }
    used = 0;
    off.clear(); len.clear(); rec.clear(); fails.clear();
    mark.clear();
    firstRec = 0xFFFFFFFFu;
    lastName.clear();
    span = nullptr;
    spanLen = 0;
    ext.clear();
    holds.clear();
    extBytes = 0;
  }
  char* room(size_t n) {  // n more bytes behind the records so far (the batch grows when a record needs it)
    if (used + n > cap) {
      const size_t want = std::max(cap * 2, used + n);
      std::unique_ptr<char[]> nb(new char[want]);
      memcpy(nb.get(), bytes.get(), used);
      bytes = std::move(nb);
      cap = want;
    }
    return bytes.get() + used;
  }
  void add(size_t n) {
    off.push_back((uint32_t)used);
    len.push_back((uint32_t)n);
    used += n;
  }
};

struct ChromIndex {  // findChrom without the linear search (first of equal names, as the search finds it)
  std::unordered_map<std::string, int> at;
  explicit ChromIndex(const State& S) {
    for (size_t i = 0; i < S.chrom.size(); i++) at.emplace(S.chrom[i].name, (int)i);
  }
  int find(const char* rname) const {
    auto it = at.find(rname);
    if (it == at.end()) die(rname, ": cannot find reference sequence name in SAM header");
    return it->second;
  }
};

// one SAM line (readSAM 4524-4560 up to the call of parseAlign)
void decodeSamLine(const Opts& o, const ChromIndex& cx, char* l, Decoded& r) {
  char* const base = l;
  if (l[0] == '@') die(l, ": misplaced SAM header line");
  // QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL [extra], cut up as the reference does
  // (readSAM 4524-4530, loadFields 4350-4377): strtok on TAB -- so a run of tabs is one separator, and
  // the last field of a line keeps its line end -- with the integer fields converted (getInt: the whole
  // token must be a number) as they are met, QUAL included in that order of events.
  char* save = nullptr;
  char* qname = strtok_r(l, "\t", &save);
  if (!qname) die(l, ": poorly formatted SAM/BAM record");
  char* fld[12] = {nullptr};
  fld[0] = qname;
  char* extra = nullptr;
  int nf = 1;
  for (char* f = strtok_r(nullptr, "\t", &save); f; f = strtok_r(nullptr, "\t", &save)) {
    fld[nf] = f;
    switch (nf) {
      case 1: r.flag = (uint16_t)getInt(f); break;
      case 3: r.pos = (uint32_t)(getInt(f) - 1); break;
      case 4: r.mapq = (uint8_t)getInt(f); break;
      case 7: r.pnext = (uint32_t)(getInt(f) - 1); break;
      case 8: (void)getInt(f); break;  // TLEN: converted, then ignored
      default: break;
    }
    if (++nf == 11) {
      extra = strtok_r(nullptr, "\n", &save);
      break;
    }
  }
  if (nf < 11) die(qname, ": poorly formatted SAM/BAM record");
  r.qname = (uint32_t)(qname - base);
  if (r.flag & 0x4) { r.kind = Decoded::UNMAPPED; return; }
  if (!strcmp(qname, "*") || !strcmp(fld[2], "*")) die(qname, ": poorly formatted SAM/BAM record");
  if (r.flag & 0xE00) { r.kind = Decoded::SUPP; return; }
  r.ci = cx.find(fld[2]);
  if (r.mapq < o.minMapQ) { r.kind = Decoded::LOWQ; return; }
  r.length = calcDist(qname, fld[9], fld[5]);
  r.score = samScore(extra);
  r.qual = (uint32_t)(fld[10] - base);
  r.qualLen = (int)strlen(fld[10]);
  r.kind = Decoded::REC;
}

// the state's side of a decoded record (the counters of readSAM / parseBAM, then parseAlign)
inline void applyDecoded(State& S, ReadSet& rs, Counts& C, const Batch& B, size_t i, int qualOffset) {
  const Decoded& r = B.rec[i];
  switch (r.kind) {
    case Decoded::FAIL: die(B.fails[(size_t)r.fail].first, B.fails[(size_t)r.fail].second.c_str());
    case Decoded::UNMAPPED: C.count++; C.unmapped++; return;
    case Decoded::SUPP: C.count++; C.supp++; return;
    case Decoded::LOWQ: C.count++; C.lowMapQ++; return;
    default: break;
  }
  C.count++;
  const char* base = B.at(i);
  record(S, rs, C, base + r.qname, r.flag, r.ci, r.pos, r.mapq, r.length, r.pnext, r.score, base + r.qual, r.qualLen, qualOffset);
}

// A span of text -> the lines gets() would have handed out, one after the other, NUL-terminated, in the batch's own
// memory (the decoders write into them): through the line feed, or REC_MAX - 1 characters of a longer line at a time.
void cutSpan(Batch& B) {
  const char* p = B.span;
  const char* const end = p + B.spanLen;
  B.clearRecords(B.spanLen + B.spanLen / 8 + REC_MAX);   // (clears span / spanLen: p and end are copies)
  while (p < end) {
    const size_t avail = std::min((size_t)(end - p), REC_MAX - 1);
    const void* nl = memchr(p, '\n', avail);
    const size_t k = nl ? (size_t)(static_cast<const char*>(nl) - p) + 1 : avail;
    char* at = B.room(k + 1);
    memcpy(at, p, k);
    at[k] = '\0';
    B.add(k + 1);
    p += k;
  }
}

// decode every record of a batch (any thread); a record that fails ends the batch: nothing behind it will be looked at
template <class F>
void decodeBatch(Batch& B, F one) {
  if (B.spanLen) cutSpan(B);
  B.rec.assign(B.off.size(), Decoded{});
  std::pair<std::string, std::string> msg;
  t_capture = &msg;
  for (size_t i = 0; i < B.off.size(); i++) {
    try {
      one(const_cast<char*>(B.at(i)), B.len[i], B.rec[i]);
    } catch (const DecodeAbort&) {
      B.rec[i].kind = Decoded::FAIL;
      B.rec[i].fail = (int)B.fails.size();
      B.fails.push_back(msg);
      B.rec.resize(i + 1);
      break;
    }
  }
  t_capture = nullptr;
  // the marks (see Batch::mark)
  const size_t n = B.rec.size();
  B.mark.resize(n);
  bool have = false;
  for (size_t i = 0; i < n; i++) {
    const Decoded& r = B.rec[i];
    uint8_t m = r.kind;
    if (r.kind == Decoded::REC) {
      const char* qname = B.at(i) + r.qname;
      if (!have) {
        have = true;
        B.firstRec = (uint32_t)i;
        B.lastName.assign(qname, strnlen(qname, MAX_ALNS));
      } else if (B.lastName == qname)  // (std::string == const char*: the whole name, as record() compares)
        m |= Batch::MARK_SAME;
      else
        B.lastName.assign(qname, strnlen(qname, MAX_ALNS));
    }
    B.mark[i] = m;
  }
}

// The pipeline: a reader thread cuts the input into batches, `nDec` threads decode them, the caller's thread takes them
// in file order.  At most `window` batches exist at a time.
class DecodePipe {
 public:
  typedef std::shared_ptr<Batch> Ptr;
  // fill(B): the reader's step -- append records to B, return false when the input is exhausted (B may hold records)
  template <class Fill, class One>
  DecodePipe(int nDec, Fill fill, One one) : window_((size_t)std::max(4, 3 * nDec)) {
    reader_ = std::thread([this, fill]() {
      for (;;) {
        Ptr b;
        {
          std::lock_guard<std::mutex> lk(m_);
          if (!free_.empty()) {
            b = free_.back();
            free_.pop_back();
          }
        }
        if (!b) b = std::make_shared<Batch>();
        const bool more = fill(*b);
        {
          std::unique_lock<std::mutex> lk(m_);
          if (b->hasWork()) {
            space_.wait(lk, [&] { return order_.size() < window_ || stop_; });
            if (stop_) break;
            order_.push_back(b);
            work_.push_back(b);
          }
          if (!more) {
            eof_ = true;
            avail_.notify_all();
            done_.notify_all();
            if (getenv("GENRICH_HOST_PROF")) {
              struct timespec ts;
              clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
              fprintf(stderr, "reader thread cpu %.3f s\n", ts.tv_sec + ts.tv_nsec * 1e-9);
            }
            break;
          }
        }
        avail_.notify_one();
      }
    });
    for (int i = 0; i < nDec; i++)
      dec_.emplace_back([this, one]() {
        for (;;) {
          Ptr b;
          {
            std::unique_lock<std::mutex> lk(m_);
            avail_.wait(lk, [&] { return !work_.empty() || eof_ || stop_; });
            if (stop_ || (work_.empty() && eof_)) return;
            b = work_.front();
            work_.pop_front();
          }
          decodeBatch(*b, one);
          {
            std::lock_guard<std::mutex> lk(m_);
            b->decoded = true;
          }
          done_.notify_all();
        }
      });
  }
  // the next batch in file order, decoded; nullptr at the end of the input
  Ptr next() {
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [&] { return (!order_.empty() && order_.front()->decoded) || (order_.empty() && eof_); });
    if (order_.empty()) return nullptr;
    Ptr b = order_.front();
    order_.pop_front();
    space_.notify_one();
    return b;
  }
  void give(Ptr b) {  // a batch the caller is done with: its memory serves the next one
    std::lock_guard<std::mutex> lk(m_);
    free_.push_back(std::move(b));
  }
  ~DecodePipe() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    space_.notify_all();
    avail_.notify_all();
    if (reader_.joinable()) reader_.join();
    for (auto& t : dec_) t.join();
  }

 private:
  std::mutex m_;
  std::condition_variable avail_, done_, space_;
  std::deque<Ptr> work_, order_;
  std::vector<Ptr> free_;
  size_t window_;
  bool eof_ = false, stop_ = false;
  std::thread reader_;
  std::vector<std::thread> dec_;
};

// reader -> decoders -> the caller's thread, or all three in turn on the caller's thread (one decoder or none)
template <class Fill, class One, class Apply>
void runDecode(int nDec, Fill fill, One one, Apply apply) {
  if (nDec > 1) {
    DecodePipe pipe(nDec, fill, one);
    while (DecodePipe::Ptr b = pipe.next()) {
      for (size_t i = 0; i < b->rec.size(); i++) apply(*b, i);
      pipe.give(std::move(b));
    }
  } else {
    Batch B;
    for (bool more = true; more;) {
      more = fill(B);
      decodeBatch(B, one);
      for (size_t i = 0; i < B.rec.size(); i++) apply(B, i);
    }
  }
}

// ---- parallel state: whole read-name groups to worker threads ---------------------------------------------------
// The decoded records still went through ONE thread's state machine (groups, pairing, weights, intervals): 15-18 M
// records/s.  But a read-name group only depends on its own records; what has an order are its RESULTS (Sink, above).
// So the thread that owns the state only (1) finds where groups begin -- a record starts a group when its name is
// not the current group's, exactly record()'s test, and skipped records (unmapped, supplementary, low MAPQ) never do --,
// (2) cuts the stream into chunks of whole groups right before such a record, and (3) merges the chunks' sinks, in
// order, into the state.  A worker runs the unchanged state machine over its chunk with a ReadSet and Counts of its
// own.  Order of events as in one thread: a chunk's last group is flushed at the chunk's end, i.e. exactly when the
// next chunk's first record -- a group start by construction -- would have flushed it; a record that fails (or a
// die() inside the state machine) ends its chunk there, with the group before it unflushed, as it ends a sequential
// run.
void addCounts(Counts& a, const Counts& b) {
  a.count += b.count; a.unmapped += b.unmapped; a.paired += b.paired; a.single += b.single; a.orphan += b.orphan;
  a.pairedPr += b.pairedPr; a.singlePr += b.singlePr; a.supp += b.supp; a.skipped += b.skipped; a.lowMapQ += b.lowMapQ;
  a.secPair += b.secPair; a.secSingle += b.secSingle;
  a.countPr += b.countPr; a.dupsPr += b.dupsPr; a.countDc += b.countDc; a.dupsDc += b.dupsDc; a.countSn += b.countSn;
  a.dupsSn += b.dupsSn;
}

struct Chunk {
  struct Seg { std::shared_ptr<Batch> b; uint32_t i0, i1; };
  std::vector<Seg> segs;
  size_t nrec = 0;
  // results
  Sink sink;
  Counts C;
  std::vector<Unpair> unpair;
  DupReads dup;
  bool failed = false;
  std::pair<std::string, std::string> fail;
  bool done = false;
};

void processChunk(State& S, Chunk& ch, int qualOffset) {
  std::pair<std::string, std::string> msg;
  t_capture = &msg;
  t_sink = &ch.sink;
  ReadSet rs;
  try {
    for (auto& sg : ch.segs)
      for (uint32_t i = sg.i0; i < sg.i1; i++) applyDecoded(S, rs, ch.C, *sg.b, i, qualOffset);
    flushSet(S, rs, ch.C);
  } catch (const DecodeAbort&) {
    ch.failed = true;
    ch.fail = msg;
  }
  t_sink = nullptr;
  t_capture = nullptr;
  ch.unpair = std::move(rs.unpair);
  ch.dup = std::move(rs.dup);
  if (!S.hot.on) ch.segs.clear();  // (the batches go as soon as nobody needs their bytes; with the int16 checks on, the owner may want them again)
}

// the state's owner takes a chunk's results (in file order)
void mergeChunk(State& S, ReadSet& rs, Counts& C, Chunk& ch, int qualOffset) {
  openSample(S);  // (record() does it at the first record that gets that far; nothing goes to the device before)
  if (S.hot.on) {
    // saveInterval's int16 checks: the chunk's events are counted; one that could be dropped, or that touches a window
    // kept exactly, sends the whole chunk through the state machine again, on this thread and in order, where every
    // read is decided as the reference decides it (the workers' results are not used)
    bool exact = false;
    for (const gx_event& e : ch.sink.ev) exact |= S.hot.add(e);
    if (exact) {
      for (const gx_event& e : ch.sink.ev) S.hot.sub(e);
      ReadSet local;  // (a chunk begins and ends between two read-name groups)
      for (auto& sg : ch.segs)
        for (uint32_t i = sg.i0; i < sg.i1; i++) applyDecoded(S, local, C, *sg.b, i, qualOffset);
      flushSet(S, local, C);
      for (auto& u : local.unpair) rs.unpair.push_back(std::move(u));
      for (auto& d : local.dup.pr) rs.dup.pr.push_back(std::move(d));
      for (auto& d : local.dup.dc) rs.dup.dc.push_back(std::move(d));
      for (auto& d : local.dup.sn) rs.dup.sn.push_back(std::move(d));
      ch.segs.clear();
      return;
    }
    ch.segs.clear();
  }
  for (auto& w : ch.sink.warn) {
    if (w.second) {
      if (S.errCount < MAX_ALNS) fputs(w.first.c_str(), stderr);
      S.errCount++;
    } else
      fputs(w.first.c_str(), stderr);
  }
  if (S.bedOpt && !ch.sink.bed.empty()) fwrite(ch.sink.bed.data(), 1, ch.sink.bed.size(), S.bed.f);
  // (the chunk's events in one piece: pushEvent's bookkeeping once per chunk, not per event)
  if (!ch.sink.ev.empty()) {
    if (!S.gx && S.hot.on) S.hot.all.insert(S.hot.all.end(), ch.sink.ev.begin(), ch.sink.ev.end());
    S.buf.insert(S.buf.end(), ch.sink.ev.begin(), ch.sink.ev.end());
    if (S.buf.size() >= (1u << 20)) {
      if (S.gx && S.sampleOpen) flushEvents(S);
      if (!S.gx || S.sampleOpen) S.buf.clear();  // (--events-only: nothing to send them to; with -b the int16 decisions keep their own copy, hot.all)
    }
  }
  if (!ch.sink.tags.empty()) {
    S.tags.insert(S.tags.end(), ch.sink.tags.begin(), ch.sink.tags.end());
    S.unpairedTags |= ch.sink.unpairedTags;
    if (S.tags.size() >= (1u << 20) && S.sampleOpen) flushTags(S);
  }
  addCounts(C, ch.C);
  for (double x : ch.sink.lenTerms) C.totalLen += x;
  for (auto& u : ch.unpair) rs.unpair.push_back(std::move(u));
  for (auto& d : ch.dup.pr) rs.dup.pr.push_back(std::move(d));
  for (auto& d : ch.dup.dc) rs.dup.dc.push_back(std::move(d));
  for (auto& d : ch.dup.sn) rs.dup.sn.push_back(std::move(d));
  if (ch.failed) die(ch.fail.first, ch.fail.second.c_str());
}

class ChunkPool {
 public:
  typedef std::shared_ptr<Chunk> Ptr;
  ChunkPool(int n, State& S, int qualOffset) {
    for (int i = 0; i < n; i++)
      th_.emplace_back([this, &S, qualOffset]() {
        for (;;) {
          Ptr c;
          {
            std::unique_lock<std::mutex> lk(m_);
            avail_.wait(lk, [&] { return !work_.empty() || stop_; });
            if (work_.empty()) return;
            c = work_.front();
            work_.pop_front();
          }
          processChunk(S, *c, qualOffset);
          {
            std::lock_guard<std::mutex> lk(m_);
            c->done = true;
          }
          done_.notify_all();
        }
      });
  }
  void submit(Ptr c) {
    {
      std::lock_guard<std::mutex> lk(m_);
      work_.push_back(c);
      order_.push_back(c);
    }
    avail_.notify_one();
  }
  // the next finished chunk in file order; with `block` waits for it, otherwise nullptr when it is not ready
  Ptr take(bool block) {
    std::unique_lock<std::mutex> lk(m_);
    if (order_.empty()) return nullptr;
    if (block) done_.wait(lk, [&] { return order_.front()->done; });
    else if (!order_.front()->done) return nullptr;
    Ptr c = order_.front();
    order_.pop_front();
    return c;
  }
  size_t pending() {
    std::lock_guard<std::mutex> lk(m_);
    return order_.size();
  }
  ~ChunkPool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
      work_.clear();
    }
    avail_.notify_all();
    for (auto& t : th_) t.join();
  }

 private:
  std::mutex m_;
  std::condition_variable avail_, done_;
  std::deque<Ptr> work_, order_;
  bool stop_ = false;
  std::vector<std::thread> th_;
};

// records per chunk (GENRICH_CHUNK_RECS: tests cut a chunk at every group)
const size_t CHUNK_RECS = getenv("GENRICH_CHUNK_RECS") ? (size_t)std::max(1L, atol(getenv("GENRICH_CHUNK_RECS"))) : (size_t)4096;
const bool g_serialState = getenv("GENRICH_SERIAL_STATE") != nullptr;  // (the one-thread state machine of before)

// reader -> decoders -> (this thread: group starts, chunks) -> workers -> (this thread: merge, in order)
template <class Fill, class One>
void runParallelState(State& S, ReadSet& rs, Counts& C, const ThreadSplit& T, int qualOffset, Fill fill, One one) {
  DecodePipe pipe(T.decode, fill, one);
  ChunkPool pool(T.state, S, qualOffset);
  const size_t window = (size_t)std::max(8, 4 * T.decode);
  std::shared_ptr<Chunk> cur = std::make_shared<Chunk>();
  bool have = false;
  std::string name;  // the current group's name as record() keeps it (the first MAX_ALNS characters)
  auto mergeReady = [&](bool block) {
    while (ChunkPool::Ptr c = pool.take(block)) mergeChunk(S, rs, C, *c, qualOffset);
  };
  while (DecodePipe::Ptr b = pipe.next()) {
    uint32_t i0 = 0;
    const uint32_t n = (uint32_t)b->rec.size();
    // A long run of records that never reach the state machine (unmapped, supplementary, low MAPQ: counters only) is
    // counted here and left out of the chunk: a chunk cannot end inside an open group, and a file that goes on for
    // millions of such records would otherwise keep all their batches in memory until the next group starts.
    constexpr uint32_t NONE = 0xFFFFFFFFu, LONG_RUN = 64;
    uint32_t runStart = NONE;
    auto endRun = [&](uint32_t i) {
      if (runStart != NONE && i - runStart >= LONG_RUN) {
        if (runStart > i0) {
          cur->segs.push_back(Chunk::Seg{b, i0, runStart});
          cur->nrec += runStart - i0;
        }
        for (uint32_t k = runStart; k < i; k++) {
          C.count++;
          const uint8_t kind = b->mark[k] & 7u;
          if (kind == Decoded::UNMAPPED) C.unmapped++;
          else if (kind == Decoded::SUPP) C.supp++;
          else C.lowMapQ++;
        }
        i0 = i;
      }
      runStart = NONE;
    };
    const uint8_t* mark = b->mark.data();
    for (uint32_t i = 0; i < n; i++) {
      const uint8_t kind = mark[i] & 7u;
      if (kind == Decoded::UNMAPPED || kind == Decoded::SUPP || kind == Decoded::LOWQ) {
        if (runStart == NONE) runStart = i;
        continue;
      }
      endRun(i);
      if (kind != Decoded::REC) continue;  // (a record that failed keeps its place in the chunk: it ends the run there)
      if (i == b->firstRec) {
        // (the batch's first record that reaches the state machine: against the name carried over from the batches before)
        const char* qname = b->at(i) + b->rec[i].qname;
        if (have && name == qname) continue;  // (std::string == const char*: the whole name, as record() compares)
      } else if (mark[i] & Batch::MARK_SAME)
        continue;
      // a group starts at record i (its name, as record() keeps it, is needed again at the next batch's first record only)
      have = true;
      if (cur->nrec + (i - i0) >= CHUNK_RECS) {
        if (i > i0) cur->segs.push_back(Chunk::Seg{b, i0, i});
        cur->nrec += i - i0;
        pool.submit(cur);
        cur = std::make_shared<Chunk>();
        i0 = i;
      }
    }
    endRun(n);
    if (b->firstRec != 0xFFFFFFFFu) name = b->lastName;  // (have is set: the first REC record either continued a group or began one)
    if (n > i0) {
      cur->segs.push_back(Chunk::Seg{b, i0, n});
      cur->nrec += n - i0;
    }
    mergeReady(false);
    while (pool.pending() > window) {  // (the workers are behind: wait for the oldest chunk rather than queue without bound)
      ChunkPool::Ptr c = pool.take(true);
      if (c) mergeChunk(S, rs, C, *c, qualOffset);
    }
  }
  if (cur->nrec) pool.submit(cur);
  while (pool.pending()) {
    ChunkPool::Ptr c = pool.take(true);
    if (c) mergeChunk(S, rs, C, *c, qualOffset);
  }
}

// a failure of the READER (a truncated BAM record ...) travels as a pseudo-record of length 0 whose bytes are the
// message: the decoder "dies" with it, and it is raised in file order like any other
void readerFailure(Batch& B, const char* tail) {
  const size_t n = strlen(tail) + 1;
  memcpy(B.room(n), tail, n);
  B.off.push_back((uint32_t)B.used);
  B.len.push_back(0u);
  B.used += n;
}

uint64_t readSAM(State& S, In& in, Counts& C, const ThreadSplit& T) {
  std::vector<char> line(REC_MAX);
  ReadSet rs;
  // the header: on this thread, line by line (it builds the table the decoders look reference names up in)
  char* l;
  while ((l = in.gets(line.data(), (int)line.size())) && l[0] == '@') headerLine(S, l);
  if (l) {
    const ChromIndex cx(S);
    const Opts& o = S.o;
    bool firstPending = true, firstOnly = true;
    auto fill = [&in, &line, &firstPending, &firstOnly](Batch& B) -> bool {
      B.reset(BATCH_BYTES + REC_MAX);
      if (firstPending) {  // (the line that ended the header)
        firstPending = false;
        const size_t n = strlen(line.data()) + 1;
        memcpy(B.room(n), line.data(), n);
        B.add(n);
      }
      if (firstOnly) {  // (the spans start with the next batch)
        firstOnly = false;
        if (!B.off.empty()) return true;
      }
      if (in.plainDirect()) {
        // a plain mapped file: the batch is the next BATCH_BYTES of it, extended to the end of the line they end in;
        // the decoder that gets it cuts it into lines (cutSpan)
        const char* p = reinterpret_cast<const char*>(in.plainPtr());
        const size_t left = in.plainLeft();
        if (!left) return false;
        size_t take = std::min(left, BATCH_BYTES);
        if (take < left) {
          const void* nl = memchr(p + take - 1, '\n', left - take + 1);
          take = nl ? (size_t)(static_cast<const char*>(nl) - p) + 1 : left;
        }
        B.span = p;
        B.spanLen = take;
        in.plainTake(take);
        return take < left;
      }
      while (B.used < BATCH_BYTES) {
        char* at = B.room(REC_MAX);
        if (!in.gets(at, (int)REC_MAX)) return false;
        B.add(strlen(at) + 1);
      }
      return true;
    };
    auto one = [&o, &cx](char* rec, uint32_t, Decoded& r) { decodeSamLine(o, cx, rec, r); };
    if (T.decode > 1 && !g_serialState)
      runParallelState(S, rs, C, T, 33, fill, one);
    else
      runDecode(T.decode, fill, one, [&](const Batch& B, size_t i) { applyDecoded(S, rs, C, B, i, 33); });
  }
  finishFile(S, rs, C);
  return C.count;
}

// ---- BAM (readBAM 4983-5068, parseBAM 4826-4977, getBAMscore 4751) -----------------------------
bool gzReadAll(In& g, void* dst, size_t n) { return n == 0 || g.read(dst, n) == n; }
// readInt32 4628-4640.  Without `must`, the end of the stream -- between records or inside the length
// field -- returns EOF (-1); so does a length field that holds -1, which the reference cannot tell apart.
int32_t rdI32(In& g, bool must) {
  uint8_t b[4];
  int k = (int)g.read(b, 4);
  if (k != 4) {
    if (!must) return -1;
    die("", "Cannot parse BAM file");
  }
  return (int32_t)(b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24));
}

float bamScore(const uint8_t* p, const uint8_t* end) {
  // getBAMscore 4751: the scan stops once fewer than five bytes remain (`while (i < len - 4)`), so a
  // one-byte-valued tag at the very end of the record is never looked at -- kept as is
  const uint8_t* stop = end - 4;
  while (p < stop) {
    const bool isAS = p[0] == 'A' && p[1] == 'S';
    const char ty = (char)p[2];
    p += 3;
    auto need = [&](size_t n) { if (p + n > end) die("", "Poorly formatted BAM auxiliary field"); };
    if (isAS && ty != 'c' && ty != 'C' && ty != 's' && ty != 'S' && ty != 'i' && ty != 'I') {
      char msg[4] = "' '";  // (an alignment score of another type -- 'A', 'f', ... -- is an error, 4782-4786)
      msg[1] = ty;
      die(msg, ": unknown value type in BAM auxiliary field");
    }
    switch (ty) {
      case 'A': case 'c': case 'C': need(1); if (isAS) return ty == 'c' ? (float)(int8_t)p[0] : (float)p[0]; p += 1; break;
      case 's': case 'S': { need(2); uint16_t v = (uint16_t)(p[0] | (p[1] << 8)); if (isAS) return ty == 's' ? (float)(int16_t)v : (float)v; p += 2; break; }
      case 'i': case 'I': { need(4); uint32_t v = p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); if (isAS) return ty == 'i' ? (float)(int32_t)v : (float)v; p += 4; break; }
      case 'f': need(4); p += 4; break;
      case 'Z': case 'H': while (p < end && *p) p++; p++; break;
      case 'B': {  // arrayLen 4712-4731
        need(5);
        char st = (char)p[0];
        size_t w;
        switch (st) {
          case 'c': case 'C': w = 1; break;
          case 's': case 'S': w = 2; break;
          case 'i': case 'I': case 'f': w = 4; break;
          default: {
            char msg[4] = "' '";
            msg[1] = st;
            die(msg, ": unknown value type in BAM auxiliary field");
          }
        }
        uint32_t cnt = p[1] | (p[2] << 8) | (p[3] << 16) | ((uint32_t)p[4] << 24);
        p += 5 + (size_t)cnt * w;
        break;
      }
      default: {
        char msg[4] = "' '";
        msg[1] = ty;
        die(msg, ": unknown value type in BAM auxiliary field");
      }
    }
  }
  return NOSCORE;
}

// the text part of a BAM header (readBAM 5007-5031): only its first line is looked at -- it must be an @HD
// line, and with the sort-order check on, one that says SO:queryname
void bamHeaderText(State& S, In& g) {
  int32_t l_text = rdI32(g, true);
  std::vector<char> text((size_t)std::max(0, l_text) + 1, 0);
  if (l_text > 0 && !gzReadAll(g, text.data(), (size_t)l_text)) die("", "Cannot parse BAM file");
  std::string firstLine(text.data(), strcspn(text.data(), "\n"));
  std::vector<char> tmp(firstLine.begin(), firstLine.end());
  tmp.push_back('\0');
  char* tag = strtok(tmp.data(), "\t");
  if (!tag || strcmp(tag, "@HD")) die("", "Cannot parse BAM file");
  const char* order = nullptr;
  for (char* f = strtok(nullptr, "\t"); f; f = strtok(nullptr, "\t"))
    if (!strncmp(f, "SO:", 3)) order = f + 3;
  if (S.o.sortOpt && (!order || strcmp(order, "queryname")))
    die("", "SAM/BAM file not sorted by queryname (samtools sort -n)");
}

// the reference table of a BAM header (readBAM, Genrich.c:5038-5049): n_ref x {l_name, name (NUL-terminated), l_ref};
// one parser for the header pre-scan and the real pass, so neither hands saveChrom an unterminated name
std::vector<int> bamRefTable(State& S, In& g) {
  int32_t n_ref = rdI32(g, true);
  std::vector<int> idx((size_t)std::max(0, n_ref));
  for (int i = 0; i < n_ref; i++) {
    int32_t len = rdI32(g, true);
    if (len < 1 || len > 65520) die("", "Cannot parse BAM file");
    std::vector<char> nm((size_t)len);
    if (!gzReadAll(g, nm.data(), (size_t)len) || nm[len - 1] != '\0') die("", "Cannot parse BAM file");
    idx[i] = saveChrom(S, nm.data(), (uint32_t)rdI32(g, true));
  }
  return idx;
}

// one BAM alignment block (parseBAM 4826-4977 up to the call of parseAlign; loadBAMfields 4660-4688)
void decodeBamBlock(const Opts& o, const std::vector<int>& idx, const char* rec, uint32_t blkLen, Decoded& r) {
  const uint8_t* blk = reinterpret_cast<const uint8_t*>(rec);
  if (blkLen == 0) die("", reinterpret_cast<const char*>(blk));  // (readerFailure)
  const int32_t n_ref = (int32_t)idx.size();
  auto i32 = [&](size_t p) { return (int32_t)(blk[p] | (blk[p + 1] << 8) | (blk[p + 2] << 16) | ((uint32_t)blk[p + 3] << 24)); };
  auto u16 = [&](size_t p) { return (uint16_t)(blk[p] | (blk[p + 1] << 8)); };
  // the name length is a signed byte, and only the end of the last field is checked against the block (4885).
  // (Offsets that leave the block on the way are an error here; the reference reads whatever its line buffer
  // holds there.)
  const int32_t refID = i32(0), pos = i32(4);
  const int l_read_name = (int8_t)blk[8];
  r.mapq = blk[9];
  const uint16_t n_cigar = u16(12);
  r.flag = u16(14);
  const int32_t l_seq = i32(16), next_pos = i32(24);
  const long long nameOff = 32, cigOff = nameOff + l_read_name, seqOff = cigOff + 4LL * n_cigar,
                  qualOff = seqOff + (l_seq + 1) / 2, auxOff = qualOff + l_seq;
  if (auxOff > (long long)blkLen) die("", "Cannot parse BAM file");
  if (cigOff < 32 || seqOff > (long long)blkLen || qualOff < 32 || qualOff > (long long)blkLen || auxOff < 32 ||
      !memchr(blk + nameOff, '\0', blkLen - (size_t)nameOff))
    die("", "Cannot parse BAM file");
  const char* qname = (const char*)&blk[nameOff];
  r.qname = (uint32_t)nameOff;
  if (r.flag & 0x4) { r.kind = Decoded::UNMAPPED; return; }
  if (!strcmp(qname, "*") || refID < 0 || refID >= n_ref || pos < 0) die(qname, ": poorly formatted SAM/BAM record");
  if (r.flag & 0xE00) { r.kind = Decoded::SUPP; return; }
  if (r.mapq < o.minMapQ) { r.kind = Decoded::LOWQ; return; }
  // calcDistBAM 4694-4706: the distance to the 3' end is l_seq - I - S + D, with no check of the CIGAR
  // against the sequence (unlike calcDist for SAM) -- also when SEQ is absent (l_seq = 0)
  int length = l_seq;
  for (int k = 0; k < n_cigar; k++) {
    const uint32_t c = (uint32_t)i32((size_t)cigOff + 4 * (size_t)k);
    const int op = (int)(c & 15);
    if (op == 1 || op == 4) length -= (int)(c >> 4);
    else if (op == 2) length += (int)(c >> 4);
  }
  r.length = length;
  r.score = bamScore(blk + (size_t)auxOff, blk + blkLen);
  r.ci = idx[(size_t)refID];
  r.pos = (uint32_t)pos;
  r.pnext = (uint32_t)next_pos;
  r.qual = (uint32_t)qualOff;
  r.qualLen = l_seq;
  r.kind = Decoded::REC;
}

uint64_t readBAM(State& S, In& in, Counts& C, const ThreadSplit& T) {
  In& g = in;
  bamHeaderText(S, g);
  const std::vector<int> idx = bamRefTable(S, g);
  ReadSet rs;
  const Opts& o = S.o;
  // the reader: alignment blocks (block_size, then that many bytes), copied out of the inflated stream
  auto fill = [&g](Batch& B) -> bool {
    B.reset(BATCH_BYTES + REC_MAX);
    const void* held = nullptr;
    // (this thread reads four bytes of every alignment block -- its size -- out of data that an inflater on another core
    // has just written: a cache miss per record, 76 ns each, was the BAM pipeline's bound on a host with many cores.
    // The member is walked front to back, so its lines are asked for 2 KiB ahead of the record being delimited.)
    const uint8_t* pf = nullptr;
    while (B.used + B.extBytes < BATCH_BYTES) {
      // (a block that lies inside one inflated BGZF member stays where it is -- the batch keeps the member alive and
      // the decoders read it there: one peek for its size, one for its bytes; one that straddles two members -- or any
      // block, with zlib's reader -- is copied through read())
      if (const uint8_t* p4 = g.peek(4)) {
        const int32_t sz = (int32_t)(p4[0] | (p4[1] << 8) | (p4[2] << 16) | ((uint32_t)p4[3] << 24));
        if (sz >= 32) {
          if (const uint8_t* whole = g.peek(4 + (size_t)sz)) {
            if (g.currentId() != held) {
              held = g.currentId();
              B.holds.push_back(g.holdCurrent());
              pf = whole;
            }
            {
              const uint8_t* const want = whole + std::min<size_t>(g.leftInCurrent(), 2048);
              if (pf < whole) pf = whole;
              for (; pf < want; pf += 64) __builtin_prefetch(pf);
            }
            B.addExt(whole + 4, (size_t)sz);
            g.advance(4 + (size_t)sz);
            continue;
          }
        }
      }
      const int32_t bs = rdI32(g, false);
      if (bs == -1) return false;  // (see rdI32)
      // (a negative size passes the reference's unsigned test and fails its end-of-block test, 4870 / 4885)
      if (bs < 32 || !gzReadAll(g, B.room((size_t)bs), (size_t)bs)) {
        readerFailure(B, "Cannot parse BAM file");
        return false;
      }
      B.add((size_t)bs);
    }
    return true;
  };
  auto one = [&o, &idx](char* rec, uint32_t len, Decoded& r) { decodeBamBlock(o, idx, rec, len, r); };
  if (T.decode > 1 && !g_serialState)
    runParallelState(S, rs, C, T, 0, fill, one);
  else
    runDecode(T.decode, fill, one, [&](const Batch& B, size_t i) { applyDecoded(S, rs, C, B, i, 0); });
  finishFile(S, rs, C);
  return C.count;
}

// ---- -v accounting (logCounts 5295-5374) -------------------------------------------------------
void logCounts(const State& S, const Counts& C, bool bam) {
  const Opts& o = S.o;
  if (S.errCount > MAX_ALNS) fprintf(stderr, "(another %ld warning messages suppressed)\n", (long)(S.errCount - MAX_ALNS));
  double avgLen = C.pairedPr ? C.totalLen / C.pairedPr : 0.0;
  fprintf(stderr, "  %s records analyzed: %11ld\n", bam ? "BAM" : "SAM", (long)C.count);
  if (C.unmapped) fprintf(stderr, "    Unmapped:           %11ld\n", (long)C.unmapped);
  if (C.supp) fprintf(stderr, "    Supp./dups/lowQual: %11ld\n", (long)C.supp);
  if (C.skipped) {
    fprintf(stderr, "    To skipped refs:    %11ld\n", (long)C.skipped);
    fprintf(stderr, "      (");
    bool first = true;
    for (auto& c : S.chrom)
      if (c.skip || !c.save) {
        fprintf(stderr, "%s%s", first ? "" : ",", c.name.c_str());
        first = false;
      }
    fprintf(stderr, ")\n");
  }
  if (C.lowMapQ) fprintf(stderr, "    MAPQ < %-2d:          %11ld\n", o.minMapQ, (long)C.lowMapQ);
  fprintf(stderr, "    Paired alignments:  %11ld\n", (long)C.paired);
  if (C.secPair) fprintf(stderr, "      secondary alns:   %11ld\n", (long)C.secPair);
  if (C.orphan) fprintf(stderr, "      \"orphan\" alns:    %11ld\t** Warning! **\n", (long)C.orphan);
  fprintf(stderr, "    Unpaired alignments:%11ld\n", (long)C.single);
  if (C.secSingle) fprintf(stderr, "      secondary alns:   %11ld\n", (long)C.secSingle);
  if (o.dupsOpt) {
    fprintf(stderr, "  PCR duplicates --\n");
    fprintf(stderr, "    Paired aln sets:    %11ld\n", (long)C.countPr);
    fprintf(stderr, "      duplicates:       %11ld (%.1f%%)\n", (long)C.dupsPr, C.countPr ? 100.0f * C.dupsPr / C.countPr : 0.0f);
    if (o.singleOpt) {
      fprintf(stderr, "    Discordant aln sets:%11ld\n", (long)C.countDc);
      fprintf(stderr, "      duplicates:       %11ld (%.1f%%)\n", (long)C.dupsDc, C.countDc ? 100.0f * C.dupsDc / C.countDc : 0.0f);
      fprintf(stderr, "    Singleton aln sets: %11ld\n", (long)C.countSn);
      fprintf(stderr, "      duplicates:       %11ld (%.1f%%)\n", (long)C.dupsSn, C.countSn ? 100.0f * C.dupsSn / C.countSn : 0.0f);
    }
  }
  fprintf(stderr, "  Fragments analyzed:   %11ld\n", (long)(C.singlePr + C.pairedPr));
  fprintf(stderr, "    Full fragments:     %11ld\n", (long)C.pairedPr);
  if (C.pairedPr && !o.atacOpt) fprintf(stderr, "      (avg. length: %.1fbp)\n", avgLen);
  if (o.singleOpt) {
    fprintf(stderr, "    Half fragments:     %11ld\n", (long)C.singlePr);
    if (C.singlePr) {
      fprintf(stderr, "      (from unpaired alns");
      if (o.extendOpt) fprintf(stderr, ", extended to %dbp", o.extend);
      else if (o.avgExtOpt && C.pairedPr) fprintf(stderr, ", extended to %dbp", (int)(avgLen + 0.5));
      fprintf(stderr, ")\n");
    }
  }
  if (o.atacOpt) {
    fprintf(stderr, "    ATAC-seq cut sites: %11ld\n", (long)(2 * C.pairedPr + C.singlePr));
    fprintf(stderr, "      (expanded to length %dbp)\n", o.atacLen5 + o.atacLen3);
  }
}

// header pre-scan: the chromosome table must be complete (in the order the reference would build
// it: first appearance over t1, c1, t2, c2, ...) before anything is sent to the device
// BAM or SAM?  checkBAM (5107-5125) looks at the first characters of a gzip-compressed input only:
// "BAM\1" is BAM; the end of the stream -- or, `char m = gzgetc()` being signed, a 0xFF byte -- before a
// character that differs from the magic is "cannot open file for reading".  Uncompressed input is SAM.
bool sniffBam(In& in, char magic[4], int& got) {
  got = (int)in.read(magic, 4);
  if (!in.compressed()) return false;
  for (int i = 0; i < 4; i++) {
    if (i >= got || (unsigned char)magic[i] == 0xFF) die("", ": cannot open file for reading");
    if (magic[i] != "BAM\1"[i]) {
      // (the reference pushes the character back with gzungetc, which refuses a negative `char`)
      if ((signed char)magic[i] < 0) die("", "Failure in ungetc() call");
      return false;
    }
  }
  return true;
}

In& openStdin(State& S) {  // openRead 5135-5166 for '-'
  if (!S.stdinIn) {
    S.stdinIn.reset(new In);
    openRead(*S.stdinIn, "-", S.threads.sam.inflate);
    if (S.stdinIn->compressed()) die("", "Cannot pipe in gzip-compressed file (use zcat instead)");
  }
  return *S.stdinIn;
}

void scanHeader(State& S, const char* filename, bool ctrl) {
  const bool isStdin = !strcmp(filename, "-");
  if (isStdin && S.stdinIn) return;  // (named twice: the second reading finds it at its end, as in the reference)
  In file;
  In& in = isStdin ? openStdin(S) : file;
  if (isStdin)
    in.record();
  else if (!in.open(filename, S.threads.sam.inflate))
    return;  // reported when the real pass gets to this file, where the reference would find out
  S.ctrl = ctrl;
  char magic[4];
  int got = 0;
  if (sniffBam(in, magic, got)) {
    bamHeaderText(S, in);
    bamRefTable(S, in);
  } else {
    in.unread(magic, (size_t)std::max(0, got));
    std::vector<char> line(65520);
    while (char* l = in.gets(line.data(), (int)line.size())) {
      if (l[0] != '@') break;
      const bool sortSave = S.o.sortOpt;
      S.o.sortOpt = false;  // the sort-order check belongs to the real pass
      headerLine(S, l);
      S.o.sortOpt = sortSave;
    }
  }
  checkIn(in);
  if (isStdin)
    in.replay();
  else
    in.close();
}

}  // namespace
