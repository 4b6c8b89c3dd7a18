// gx_peak_merge.h -- which peak is peak_N: the peak lists of several contexts (chromosomes sharded over GPUs) merged into the order
// of the narrowPeak file, and what a per-peak writer's payload needs to follow them: a column permuted, indexed records renumbered.
// Every writer with one row (or one group of rows) per peak numbers its peaks through this, so peak_N names the same peak in every
// file of a run.  Host only, nothing of the library's but its types (and merged_peaks' declaration): tests/peak_merge_main.cpp
// compiles it alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/genrich_amd.h"

namespace gx_peak_merge {

// The lists concatenated in list order, then -- for more than one list -- stable-sorted by (chrom, start): chromosome-table order,
// then position, the order in which the reference meets the peaks (Genrich.c:986, 925).  One list is left as it is (a context's
// own list is in that order already).  Merged peak i is peak_i.
struct Merged {
  std::vector<gx_peak> peaks;       // in output order
  std::vector<gx_region> regions;   // ... as the formatters take them
  std::vector<size_t> from;         // from[i]: where merged peak i stands in the concatenation
  std::vector<size_t> rank;         // rank[j]: the merged index of concatenated peak j (the inverse of from)
  std::vector<size_t> first;        // first[g]: where list g begins in the concatenation (first[n_lists]: its end): peak k of list g
                                    // is merged peak rank[first[g] + k]
  size_t size() const { return peaks.size(); }
};

inline Merged merge(const gx_peak* const* lists, const size_t* n, size_t n_lists) {
  Merged m;
  std::vector<gx_peak> all;
  for (size_t g = 0; g < n_lists; g++) {
    m.first.push_back(all.size());
    all.insert(all.end(), lists[g], lists[g] + n[g]);
  }
  m.first.push_back(all.size());
  m.from.resize(all.size());
  for (size_t i = 0; i < all.size(); i++) m.from[i] = i;
  if (n_lists > 1)
    std::stable_sort(m.from.begin(), m.from.end(), [&](size_t a, size_t b) {
      return all[a].chrom != all[b].chrom ? all[a].chrom < all[b].chrom : all[a].start < all[b].start;
    });
  m.rank.resize(all.size());
  for (size_t i = 0; i < all.size(); i++) {
    const gx_peak& p = all[m.from[i]];
    m.peaks.push_back(p);
    m.regions.push_back(gx_region{p.chrom, p.start, p.end});
    m.rank[m.from[i]] = i;
  }
  return m;
}

// ... of the lists of contexts, through gx_peak_count / gx_get_peaks (gx_emit.cpp, beside the narrowPeak writer; a status of theirs)
int merged_peaks(gx_ctx* const* ctxs, int n_ctx, Merged& m);

// A per-peak column that came in concatenation order (list after list), in merged order
template <class T>
std::vector<T> permuted(const Merged& m, const std::vector<T>& col) {
  std::vector<T> out(m.size());
  for (size_t i = 0; i < out.size(); i++) out[i] = col[m.from[i]];
  return out;
}

// (peak, less): the order of records that carry a peak index, less ordering those of one peak
template <class R, class Less>
auto by_peak(uint32_t R::*peak, Less less) {
  return [=](const R& a, const R& b) { return a.*peak != b.*peak ? a.*peak < b.*peak : less(a, b); };
}

// Records that name a peak by its index in their own list (recs[g]: list g's, R::*peak the index): all of them with the merged
// index instead, list after list; for more than one list sorted by_peak -- one list's records are taken to come in that order already.
template <class R, class Less>
std::vector<R> renumbered(const Merged& m, const std::vector<std::vector<R>>& recs, uint32_t R::*peak, Less less) {
  std::vector<R> out;
  for (size_t g = 0; g < recs.size(); g++)
    for (R r : recs[g]) {
      r.*peak = (uint32_t)m.rank[m.first[g] + r.*peak];
      out.push_back(r);
    }
  if (recs.size() > 1) std::sort(out.begin(), out.end(), by_peak(peak, less));
  return out;
}

// The order of a peak's summits and of a peak's motif hits (the latter also sorts a context's own scan: mot_pass)
inline bool summit_less(const gx_summit& a, const gx_summit& b) { return a.pos < b.pos; }
inline bool motif_hit_less(const gx_motif_hit& x, const gx_motif_hit& y) {
  if (x.pos != y.pos) return x.pos < y.pos;
  if (x.motif != y.motif) return x.motif < y.motif;
  return x.strand < y.strand;
}

}  // namespace gx_peak_merge
