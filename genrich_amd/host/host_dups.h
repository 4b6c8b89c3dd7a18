// host_dups.h -- -r / -R: the alignment sets kept to the end of the file and the PCR duplicates among them (findDups).
// (a part of genrich_amd.cpp's translation unit)
#pragma once
namespace {

// ---- -r: alignment sets kept until the end of the file (saveAlns 2942-2977) --------------------
struct DRead {
  std::string name;
  uint16_t qual = 0;            // sum of the base qualities (both mates for pairs / discordant pairs)
  bool first = false;           // singleton: which mate
  float score = NOSCORE, scoreR2 = NOSCORE;
  std::vector<Aln> aln, alnR2;  // alnR2: the R2 alignments of a discordant pair
};
struct DupReads { std::vector<DRead> pr, dc, sn; };

// copyAlns 2815-2851: the unpaired alignments of one mate within the score window
void copyAlns(const State& S, const std::vector<Aln>& aln, float score, bool first, std::vector<Aln>& dest) {
  if (score != NOSCORE) score -= S.o.asDiff;
  for (auto& a : aln)
    if (!a.paired && a.first == first && a.score >= score) dest.push_back(a);
}

void saveAlns(const State& S, const char* qname, const std::vector<Aln>& aln, bool pair, bool singleR1, bool singleR2,
              float scorePr, float scoreR1, float scoreR2, uint16_t qualR1, uint16_t qualR2, DupReads& D) {
  auto sumq = [](uint16_t a, uint16_t b) { return (uint16_t)std::min<int>((int)a + (int)b, UINT16_MAX); };
  if (pair) {  // saveAlnsPair 2890-2935: positions ordered
    DRead r;
    r.name = qname;
    r.qual = sumq(qualR1, qualR2);
    r.score = scorePr;
    float score = scorePr;
    if (score != NOSCORE) score -= S.o.asDiff;
    for (auto& a : aln)
      if (a.paired && a.full && a.score >= score) {
        Aln b = a;
        if (b.pos[0] > b.pos[1]) std::swap(b.pos[0], b.pos[1]);
        r.aln.push_back(b);
      }
    D.pr.push_back(std::move(r));
  } else if (S.o.singleOpt) {
    if (singleR1 && singleR2) {  // both mates aligned, not as a proper pair (saveAlnsDiscord 2874)
      DRead r;
      r.name = qname;
      r.first = true;
      r.score = scoreR1;
      r.scoreR2 = scoreR2;
      copyAlns(S, aln, scoreR1, true, r.aln);
      copyAlns(S, aln, scoreR2, false, r.alnR2);
      r.qual = sumq(qualR1, qualR2);
      D.dc.push_back(std::move(r));
    } else if (singleR1 || singleR2) {  // saveAlnsSingle 2856
      DRead r;
      r.name = qname;
      r.first = singleR1;
      r.score = singleR1 ? scoreR1 : scoreR2;
      r.qual = singleR1 ? qualR1 : qualR2;
      copyAlns(S, aln, r.score, r.first, r.aln);
      D.sn.push_back(std::move(r));
    }
  }
}

// ---- -r: PCR duplicates (findDups 3949-4042) ---------------------------------------------------
// Sets are visited from the highest base-quality sum down (a stable order, sortReads 3362); a set
// is a duplicate when any of its alignments matches one already kept: proper pairs by (chrom,
// both 5' ends), discordant pairs by both ends with their strands in either order, singletons by
// (chrom, 5' end, strand) -- against kept singletons and against both ends of every kept pair.
// Only membership matters, so ordered maps stand in for the reference's chained hash tables.
// (hash tables, as the reference's: only "is this key there, and who put it there first" is ever asked -- an ordered
// map of 10^7 keys made findDups the slowest part of a -r run)
struct KeyPr { int chrom; uint32_t p0, p1; bool operator==(const KeyPr& o) const { return chrom == o.chrom && p0 == o.p0 && p1 == o.p1; } };
struct KeySn { int chrom; uint32_t pos; bool strand; bool operator==(const KeySn& o) const { return chrom == o.chrom && pos == o.pos && strand == o.strand; } };
struct KeyDc {
  int c0, c1; uint32_t p0, p1; bool s0, s1;
  bool operator==(const KeyDc& o) const { return c0 == o.c0 && c1 == o.c1 && p0 == o.p0 && p1 == o.p1 && s0 == o.s0 && s1 == o.s1; }
};
inline uint64_t mix64(uint64_t x) {  // (splitmix64's finaliser)
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31;
  return x;
}
struct KeyHash {
  size_t operator()(const KeyPr& k) const { return (size_t)mix64(((uint64_t)k.p0 << 32 | k.p1) ^ mix64((uint64_t)(uint32_t)k.chrom)); }
  size_t operator()(const KeySn& k) const { return (size_t)mix64(((uint64_t)k.pos << 1 | (uint64_t)k.strand) ^ mix64((uint64_t)(uint32_t)k.chrom + 0x9e3779b97f4a7c15ull)); }
  size_t operator()(const KeyDc& k) const {
    return (size_t)mix64(((uint64_t)k.p0 << 32 | k.p1) ^ mix64(((uint64_t)(uint32_t)k.c0 << 32 | (uint32_t)k.c1) ^ ((uint64_t)k.s0 << 1 | (uint64_t)k.s1)));
  }
};

void dupLine(State& S, const char* fmt, ...) {
  char buf[2 * MAX_ALNS + 4096];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  fputs(buf, S.dups.f);
}

// Who held a key first -- the membership half of the tables -- comes from the device when there is one
// (gx_dups_first, gx_dups.h): every alignment of the file's sets at once instead of one hash probe after the other.
// What it cannot decide (sets with several alignments give up all their keys when one matches; whatever shares a key
// with such a set is "contested") is walked here in the reference's order, on tables that hold the contested keys only.
struct DupDevice {
  bool on = false;
  std::vector<gx_dup_key> keys;
  std::vector<uint8_t> multi;
  std::vector<uint32_t> owner, readOf;   // per record: gx_dups_first's word; the set (or addition) it belongs to
  uint64_t nKeys = 0, nContested = 0, nByTable[4] = {0, 0, 0, 0};   // (by the key's tag: 1 proper pairs, 2 discordant, 3 singletons)
  uint64_t nContBy[4] = {0, 0, 0, 0}, nContAdds = 0;   // the contested records by tag; of the singleton table's, the additions apart
  void clear() { keys.clear(); multi.clear(); owner.clear(); readOf.clear(); }
  void push(uint32_t tag, uint32_t a, uint32_t b, uint32_t c, bool m, uint32_t read) {
    keys.push_back(gx_dup_key{{tag, a, b, c}});
    multi.push_back(m ? 1 : 0);
    readOf.push_back(read);
  }
};
constexpr uint32_t DUP_CONTESTED = 0x80000000u;

void findDups(State& S, DupReads& D, Counts& C) {
  const bool verb = S.dupsVerb;
  std::unordered_map<KeySn, std::string, KeyHash> tabSn;
  const bool useSn = S.o.singleOpt && !D.sn.empty();  // the singleton table exists only when there are singletons
  DupDevice dev;
  dev.on = S.gx && !S.devs.ctx.empty() && !getenv("GENRICH_DUPS_HOST");
  // device mode: what checkAndAdd (3514) puts into the singleton table ahead of the singletons -- both ends of every
  // kept pair -- is a list of records that lead the singletons' own (the table's first holder of a key names the read)
  struct SnAdd { int chrom; uint32_t pos; bool strand; std::string name; };
  std::vector<SnAdd> snAdds;
  auto addSn = [&](int chrom, uint32_t pos, bool strand, const std::string& name) {  // checkAndAdd 3514
    if (dev.on) snAdds.push_back(SnAdd{chrom, pos, strand, verb ? name : std::string()});
    else tabSn.emplace(KeySn{chrom, pos, strand}, verb ? name : std::string());
  };
  auto order = [](const std::vector<DRead>& v) {
    std::vector<uint32_t> o(v.size());
    for (uint32_t i = 0; i < o.size(); i++) o[i] = i;
    std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return v[a].qual > v[b].qual; });
    return o;
  };
  auto runDevice = [&](size_t nAdds = 0) {   // (nAdds: the records that lead the batch and are additions, not sets)
    dev.owner.assign(dev.keys.size(), 0);
    if (!dev.keys.empty())
      check(S, gx_dups_first(S.devs.ctx[0], dev.keys.data(), dev.multi.data(), dev.keys.size(), dev.owner.data()), S.devs.ctx[0]);
    dev.nKeys += dev.keys.size();
    for (const gx_dup_key& k : dev.keys) dev.nByTable[k.w[0] & 3u]++;   // (per key: a batch need not hold one table's keys)
    for (size_t i = 0; i < dev.owner.size(); i++)
      if (dev.owner[i] & DUP_CONTESTED) {
        dev.nContested++;
        if (i < nAdds) dev.nContAdds++;
        else dev.nContBy[dev.keys[i].w[0] & 3u]++;
      }
  };
  auto report = [&]() {
    if (!dev.on || !getenv("GENRICH_DUPS_REPORT")) return;
    fprintf(stderr, "[dups] device: %llu keys, %llu contested (resolved on the host); by table: %llu paired, %llu discordant, %llu single\n",
            (unsigned long long)dev.nKeys, (unsigned long long)dev.nContested, (unsigned long long)dev.nByTable[1],
            (unsigned long long)dev.nByTable[2], (unsigned long long)dev.nByTable[3]);
    fprintf(stderr, "[dups] contested: %llu paired, %llu discordant, %llu single, %llu additions\n", (unsigned long long)dev.nContBy[1],
            (unsigned long long)dev.nContBy[2], (unsigned long long)dev.nContBy[3], (unsigned long long)dev.nContAdds);
  };

  {  // properly paired sets (findDupsPr 3616)
    std::unordered_map<KeyPr, std::string, KeyHash> tab;   // (device mode: the contested keys only)
    const std::vector<uint32_t> ord = order(D.pr);
    std::vector<uint32_t> firstRec;
    if (dev.on) {
      firstRec.resize(ord.size() + 1);
      for (size_t q = 0; q < ord.size(); q++) {
        const DRead& r = D.pr[ord[q]];
        firstRec[q] = (uint32_t)dev.keys.size();
        for (auto& a : r.aln) dev.push(1u, (uint32_t)a.chrom, a.pos[0], a.pos[1], r.aln.size() > 1, ord[q]);
      }
      firstRec[ord.size()] = (uint32_t)dev.keys.size();
      runDevice();
    }
    for (size_t q = 0; q < ord.size(); q++) {
      DRead& r = D.pr[ord[q]];
      bool dup = false;
      const bool byDevice = dev.on && r.aln.size() == 1 && !(dev.owner[firstRec[q]] & DUP_CONTESTED);
      if (byDevice) {
        const uint32_t me = firstRec[q], own = dev.owner[me];
        if (own != me) {
          const Aln& a = r.aln[0];
          if (verb) dupLine(S, "%s\t%s:%d-%d\t%s\tpaired\n", r.name.c_str(), S.chrom[a.chrom].name.c_str(), a.pos[0], a.pos[1],
                            D.pr[dev.readOf[own]].name.c_str());
          dup = true;
        }
      } else
      for (auto& a : r.aln) {
        auto it = tab.find(KeyPr{a.chrom, a.pos[0], a.pos[1]});
        if (it != tab.end()) {
          if (verb) dupLine(S, "%s\t%s:%d-%d\t%s\tpaired\n", r.name.c_str(), S.chrom[a.chrom].name.c_str(), a.pos[0], a.pos[1], it->second.c_str());
          dup = true;
          break;
        }
      }
      if (dup) C.dupsPr++;
      else {
        for (auto& a : r.aln) {
          if (!byDevice) tab.emplace(KeyPr{a.chrom, a.pos[0], a.pos[1]}, verb ? r.name : std::string());
          if (useSn) {
            addSn(a.chrom, a.pos[0], true, r.name);
            addSn(a.chrom, a.pos[1], false, r.name);
          }
        }
        C.pairedPr += processPair(S, r.name.c_str(), r.aln, C, r.score);
      }
      C.countPr++;
    }
    D.pr.clear();
    D.pr.shrink_to_fit();
    dev.clear();
  }
  if (!S.o.singleOpt) {
    report();
    return;
  }

  // with -x the average fragment length of the kept pairs becomes the extension (3990-3996)
  const Opts saved = S.o;
  if (S.o.avgExtOpt) {
    int extend = 0;
    if (!C.pairedPr) {
      if (S.o.verbose) {
        fprintf(stderr, "Warning! No paired alignments to calculate avg frag ");
        fprintf(stderr, "length --\n  Printing unpaired alignments \"as is\"\n");
      }
    } else
      extend = (int)(C.totalLen / C.pairedPr + 0.5);
    S.o.extend = extend;
    if (extend) S.o.extendOpt = true;
    S.o.avgExtOpt = false;
  }
  std::vector<Unpair> none;

  {  // discordant sets (findDupsDc 3761): every R1 x R2 combination, either order
    std::unordered_map<KeyDc, std::string, KeyHash> tab;   // (device mode: the contested keys only)
    auto end5 = [](const Aln& a) { return a.strand ? a.pos[0] : a.pos[1]; };
    const std::vector<uint32_t> ord = order(D.dc);
    // Device mode: the reference looks a combination up in both orders and stores it in one (3786-3837), i.e. the table is
    // keyed on the UNORDERED pair of ends -- one record per combination with the two ends in a canonical order.  The
    // chromosomes share a word: genomes of more than 65,536 sequences keep the host's tables.
    const bool dcDev = dev.on && S.chrom.size() <= 65536;
    if (dev.on && !dcDev && !D.dc.empty() && getenv("GENRICH_DUPS_REPORT"))
      fprintf(stderr, "[dups] discordant sets: the host's tables (more than 65,536 sequences: two chromosome indices do not fit a key word)\n");
    std::vector<uint32_t> firstRec;
    auto canon = [&](const Aln& a, const Aln& b, uint32_t w[4]) {
      const uint32_t pa = end5(a), pb = end5(b);
      const bool swap = std::make_tuple(b.chrom, pb, (int)b.strand) < std::make_tuple(a.chrom, pa, (int)a.strand);
      const Aln &x = swap ? b : a, &y = swap ? a : b;
      w[0] = 2u | ((uint32_t)x.strand << 8) | ((uint32_t)y.strand << 9);
      w[1] = (uint32_t)x.chrom | ((uint32_t)y.chrom << 16);
      w[2] = swap ? pb : pa;
      w[3] = swap ? pa : pb;
    };
    if (dcDev) {
      firstRec.resize(ord.size() + 1);
      for (size_t q = 0; q < ord.size(); q++) {
        const DRead& r = D.dc[ord[q]];
        firstRec[q] = (uint32_t)dev.keys.size();
        const bool multi = r.aln.size() * r.alnR2.size() > 1;
        for (auto& a : r.aln)
          for (auto& b : r.alnR2) {
            uint32_t w[4];
            canon(a, b, w);
            dev.keys.push_back(gx_dup_key{{w[0], w[1], w[2], w[3]}});
            dev.multi.push_back(multi ? 1 : 0);
            dev.readOf.push_back(ord[q]);
          }
      }
      firstRec[ord.size()] = (uint32_t)dev.keys.size();
      runDevice();
    }
    for (size_t q = 0; q < ord.size(); q++) {
      DRead& r = D.dc[ord[q]];
      bool dup = false;
      const bool byDevice = dcDev && r.aln.size() == 1 && r.alnR2.size() == 1 && !(dev.owner[firstRec[q]] & DUP_CONTESTED);
      if (byDevice) {
        const uint32_t me = firstRec[q], own = dev.owner[me];
        if (own != me) {
          // (an uncontested key: its first holder is a set of one combination too, stored as (its R1, its R2); the
          // reference finds it in the order of this set's ends first, in the swapped order otherwise -- 3786 / 3812)
          const DRead& hr = D.dc[dev.readOf[own]];
          const Aln &a = r.aln[0], &b = r.alnR2[0], &ha = hr.aln[0], &hb = hr.alnR2[0];
          const uint32_t pos = end5(a), pos1 = end5(b);
          const bool sameOrder = ha.chrom == a.chrom && hb.chrom == b.chrom && end5(ha) == pos && end5(hb) == pos1 &&
                                 ha.strand == a.strand && hb.strand == b.strand;
          if (verb) {
            if (sameOrder)
              dupLine(S, "%s\t%s:%d,%c;%s:%d,%c\t%s\tdiscordant\n", r.name.c_str(), S.chrom[a.chrom].name.c_str(), pos,
                      a.strand ? '+' : '-', S.chrom[b.chrom].name.c_str(), pos1, b.strand ? '+' : '-', hr.name.c_str());
            else
              dupLine(S, "%s\t%s:%d,%c;%s:%d,%c\t%s\tdiscordant\n", r.name.c_str(), S.chrom[b.chrom].name.c_str(), pos1,
                      b.strand ? '+' : '-', S.chrom[a.chrom].name.c_str(), pos, a.strand ? '+' : '-', hr.name.c_str());
          }
          dup = true;
        }
      } else
      for (size_t k = 0; k < r.aln.size() && !dup; k++) {
        const Aln& a = r.aln[k];
        const uint32_t pos = end5(a);
        for (size_t j = 0; j < r.alnR2.size() && !dup; j++) {
          const Aln& b = r.alnR2[j];
          const uint32_t pos1 = end5(b);
          auto it = tab.find(KeyDc{a.chrom, b.chrom, pos, pos1, a.strand, b.strand});
          if (it != tab.end()) {
            if (verb) dupLine(S, "%s\t%s:%d,%c;%s:%d,%c\t%s\tdiscordant\n", r.name.c_str(), S.chrom[a.chrom].name.c_str(), pos,
                              a.strand ? '+' : '-', S.chrom[b.chrom].name.c_str(), pos1, b.strand ? '+' : '-', it->second.c_str());
            dup = true;
            break;
          }
          it = tab.find(KeyDc{b.chrom, a.chrom, pos1, pos, b.strand, a.strand});
          if (it != tab.end()) {
            if (verb) dupLine(S, "%s\t%s:%d,%c;%s:%d,%c\t%s\tdiscordant\n", r.name.c_str(), S.chrom[b.chrom].name.c_str(), pos1,
                              b.strand ? '+' : '-', S.chrom[a.chrom].name.c_str(), pos, a.strand ? '+' : '-', it->second.c_str());
            dup = true;
          }
        }
      }
      if (dup) C.dupsDc++;
      else {
        for (size_t k = 0; k < r.aln.size(); k++)
          for (size_t j = 0; j < r.alnR2.size(); j++) {
            const Aln &a = r.aln[k], &b = r.alnR2[j];
            if (!byDevice) tab.emplace(KeyDc{a.chrom, b.chrom, end5(a), end5(b), a.strand, b.strand}, verb ? r.name : std::string());
            if (useSn) {
              if (!j) addSn(a.chrom, end5(a), a.strand, r.name);
              if (!k) addSn(b.chrom, end5(b), b.strand, r.name);
            }
          }
        C.singlePr += processSingle(S, r.name.c_str(), r.aln, none, r.score, true);
        C.singlePr += processSingle(S, r.name.c_str(), r.alnR2, none, r.scoreR2, false);
      }
      C.countDc++;
    }
    D.dc.clear();
    D.dc.shrink_to_fit();
    dev.clear();
  }

  {  // singletons (findDupsSn 3886): the table already holds the ends of the kept pairs
    auto end5 = [](const Aln& a) { return a.strand ? a.pos[0] : a.pos[1]; };
    const std::vector<uint32_t> ord = order(D.sn);
    std::vector<uint32_t> firstRec;
    const uint32_t nAdds = (uint32_t)snAdds.size();
    if (dev.on) {
      // the additions first (never duplicates themselves: they only take a key if it is free), then the singletons
      for (uint32_t k = 0; k < nAdds; k++) dev.push(3u, (uint32_t)snAdds[k].chrom, snAdds[k].pos, snAdds[k].strand, false, k);
      firstRec.resize(ord.size() + 1);
      for (size_t q = 0; q < ord.size(); q++) {
        const DRead& r = D.sn[ord[q]];
        firstRec[q] = (uint32_t)dev.keys.size();
        for (auto& a : r.aln) dev.push(3u, (uint32_t)a.chrom, end5(a), a.strand, r.aln.size() > 1, nAdds + ord[q]);
      }
      firstRec[ord.size()] = (uint32_t)dev.keys.size();
      runDevice(nAdds);
      // the contested keys among the additions enter the host's table, in their order (the first holder stays)
      for (uint32_t k = 0; k < nAdds; k++)
        if (dev.owner[k] & DUP_CONTESTED) tabSn.emplace(KeySn{snAdds[k].chrom, snAdds[k].pos, snAdds[k].strand}, snAdds[k].name);
    }
    auto holder = [&](uint32_t rec) -> const std::string& {  // the read that put record rec's key there
      const uint32_t id = dev.readOf[rec];
      return id < nAdds ? snAdds[id].name : D.sn[id - nAdds].name;
    };
    for (size_t q = 0; q < ord.size(); q++) {
      DRead& r = D.sn[ord[q]];
      bool dup = false;
      const bool byDevice = dev.on && r.aln.size() == 1 && !(dev.owner[firstRec[q]] & DUP_CONTESTED);
      if (byDevice) {
        const uint32_t me = firstRec[q], own = dev.owner[me];
        if (own != me) {
          const Aln& a = r.aln[0];
          if (verb) dupLine(S, "%s\t%s:%d,%c\t%s\tsingle\n", r.name.c_str(), S.chrom[a.chrom].name.c_str(), end5(a),
                            a.strand ? '+' : '-', holder(own).c_str());
          dup = true;
        }
      } else
      for (auto& a : r.aln) {
        auto it = tabSn.find(KeySn{a.chrom, end5(a), a.strand});
        if (it != tabSn.end()) {
          if (verb) dupLine(S, "%s\t%s:%d,%c\t%s\tsingle\n", r.name.c_str(), S.chrom[a.chrom].name.c_str(), end5(a),
                            a.strand ? '+' : '-', it->second.c_str());
          dup = true;
          break;
        }
      }
      if (dup) C.dupsSn++;
      else {
        if (!byDevice)
          for (auto& a : r.aln) tabSn.emplace(KeySn{a.chrom, end5(a), a.strand}, verb ? r.name : std::string());
        C.singlePr += processSingle(S, r.name.c_str(), r.aln, none, r.score, r.first);
      }
      C.countSn++;
    }
    D.sn.clear();
    D.sn.shrink_to_fit();
    dev.clear();
  }
  report();
  S.o = saved;
}

}  // namespace
