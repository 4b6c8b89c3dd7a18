// peak_merge_main.cpp -- gx_peak_merge.h alone, for tests/test_peak_merge.py (compiled with the sanitizers).  stdin holds cases:
//   case L
//   then per list:  list N H S | N lines `chrom start end summit value` | H lines `peak pos motif strand score` | S lines `peak pos`
// (value: a per-peak column; the hits and the summits name a peak by its index in their own list).  Per case the merged peaks,
// from, rank, first, the column in merged order, the hits and the summits renumbered; "--" ends a case.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../genrich_amd/csrc/gx_peak_merge.h"

int main() {
  size_t L = 0;
  while (scanf(" case %zu", &L) == 1) {
    std::vector<std::vector<gx_peak>> peaks(L);
    std::vector<std::vector<gx_motif_hit>> hits(L);
    std::vector<std::vector<gx_summit>> sums(L);
    std::vector<int64_t> column;   // in concatenation order
    for (size_t g = 0; g < L; g++) {
      size_t N = 0, H = 0, S = 0;
      if (scanf(" list %zu %zu %zu", &N, &H, &S) != 3) return 2;
      for (size_t i = 0; i < N; i++) {
        gx_peak p{};
        int64_t v = 0;
        if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNd64, &p.chrom, &p.start, &p.end, &p.summit, &v) != 5) return 2;
        peaks[g].push_back(p);
        column.push_back(v);
      }
      for (size_t i = 0; i < H; i++) {
        gx_motif_hit h{};
        unsigned motif = 0, strand = 0;
        if (scanf("%" SCNu32 " %" SCNu32 " %u %u %" SCNd32, &h.region, &h.pos, &motif, &strand, &h.score) != 5) return 2;
        h.motif = (uint16_t)motif;
        h.strand = (uint8_t)strand;
        hits[g].push_back(h);
      }
      for (size_t i = 0; i < S; i++) {
        gx_summit s{};
        if (scanf("%" SCNu32 " %" SCNu32, &s.peak, &s.pos) != 2) return 2;
        sums[g].push_back(s);
      }
    }
    std::vector<const gx_peak*> lists;
    std::vector<size_t> n;
    for (const std::vector<gx_peak>& l : peaks) {
      lists.push_back(l.data());
      n.push_back(l.size());
    }
    const gx_peak_merge::Merged m = gx_peak_merge::merge(lists.data(), n.data(), L);
    if (m.regions.size() != m.size() || m.from.size() != m.size() || m.rank.size() != m.size() || m.first.size() != L + 1) return 3;
    printf("peaks\n");
    for (size_t i = 0; i < m.size(); i++) {
      const gx_peak& p = m.peaks[i];
      const gx_region& r = m.regions[i];
      if (r.chrom != p.chrom || r.start != p.start || r.end != p.end) return 3;
      printf("%u %u %u %u\n", p.chrom, p.start, p.end, p.summit);
    }
    printf("from\n");
    for (size_t v : m.from) printf("%zu\n", v);
    printf("rank\n");
    for (size_t v : m.rank) printf("%zu\n", v);
    printf("first\n");
    for (size_t v : m.first) printf("%zu\n", v);
    printf("column\n");
    for (int64_t v : gx_peak_merge::permuted(m, column)) printf("%" PRId64 "\n", v);
    printf("hits\n");
    for (const gx_motif_hit& h : gx_peak_merge::renumbered(m, hits, &gx_motif_hit::region, gx_peak_merge::motif_hit_less))
      printf("%u %u %u %u %d\n", h.region, h.pos, (unsigned)h.motif, (unsigned)h.strand, h.score);
    printf("summits\n");
    for (const gx_summit& s : gx_peak_merge::renumbered(m, sums, &gx_summit::peak, gx_peak_merge::summit_less)) printf("%u %u\n", s.peak, s.pos);
    printf("--\n");
  }
  return 0;
}
