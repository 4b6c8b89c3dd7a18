// Stand-alone driver of gx_rank_tables (genrich_amd/csrc/gx_emit.cpp) for tests/test_spearman.py, which compiles it together
// with gx_emit.cpp under -fsanitize=address,undefined and compares its output with tests/rank_ref.py.  No device and no
// library: the C ABI entries gx_emit.cpp's writers call are defined here and never reached.
//
// Spec file (argv[1]): per case one line "G S n_zero_to_drop", then G * S tables (context after context, sample after sample),
// each a line "n" followed by n lines "value count".  Output (stdout): per case "rc N", and when rc is 0 per sample a line "D"
// followed by D lines "value rank2"; every case is followed by "--\n".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../include/genrich_amd.h"

struct gx_ctx { int unused; };

extern "C" {
int gx_peak_count(gx_ctx*, size_t*) { return GX_ERR_ORDER; }
int gx_get_peaks(gx_ctx*, gx_peak*, size_t) { return GX_ERR_ORDER; }
int gx_get_peak_counts(gx_ctx*, int, int*, int*, int64_t*, size_t, int64_t*, int64_t*) { return GX_ERR_ORDER; }
int gx_get_region_counts(gx_ctx*, int, int*, int*, int64_t*, size_t, int64_t*, int64_t*) { return GX_ERR_ORDER; }
int gx_interval_count(gx_ctx*, int, int, size_t*) { return GX_ERR_ORDER; }
int gx_get_intervals(gx_ctx*, int, int, size_t, uint32_t*, float*, float*, float*, float*) { return GX_ERR_ORDER; }
int gx_coverage_bin_count(gx_ctx*, int, size_t*) { return GX_ERR_ORDER; }
int gx_coverage_layout(gx_ctx*, int, uint32_t*, uint32_t*) { return GX_ERR_ORDER; }
int gx_get_coverage(gx_ctx*, int, int, int*, int*, int64_t*, size_t) { return GX_ERR_ORDER; }
}

// (exact-size heap arrays: a read or a write beyond them is the sanitizer's to catch)
typedef std::unique_ptr<uint64_t[]> Arr;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  for (;;) {
    int G = 0, S = 0;
    uint64_t drop = 0;
    if (fscanf(f, "%d %d %" SCNu64, &G, &S, &drop) != 3) break;
    const size_t T = (size_t)G * S;
    std::vector<Arr> vals(T), cnts(T);
    std::vector<gx_rank_table> tabs(T);
    for (size_t t = 0; t < T; t++) {
      size_t n = 0;
      if (fscanf(f, "%zu", &n) != 1) return 2;
      vals[t].reset(new uint64_t[n]);
      cnts[t].reset(new uint64_t[n]);
      for (size_t k = 0; k < n; k++)
        if (fscanf(f, "%" SCNu64 " %" SCNu64, &vals[t][k], &cnts[t][k]) != 2) return 2;
      tabs[t] = gx_rank_table{n ? vals[t].get() : nullptr, n ? cnts[t].get() : nullptr, n};
    }
    std::vector<size_t> nOut((size_t)S, 0);
    uint64_t N = 0;
    int rc = gx_rank_tables(G, S, tabs.data(), drop, nullptr, nullptr, 0, nOut.data(), &N);   // the sizes first
    std::vector<Arr> ov((size_t)S), orr((size_t)S);
    std::vector<uint64_t*> pv((size_t)S), pr((size_t)S);
    size_t cap = 0;
    if (!rc) {
      for (int s = 0; s < S; s++) cap = nOut[s] > cap ? nOut[s] : cap;
      for (int s = 0; s < S; s++) {
        ov[s].reset(new uint64_t[cap]);
        orr[s].reset(new uint64_t[cap]);
        pv[s] = ov[s].get();
        pr[s] = orr[s].get();
      }
      if (cap && gx_rank_tables(G, S, tabs.data(), drop, pv.data(), pr.data(), cap - 1, nOut.data(), &N) != GX_ERR_ORDER) return 3;   // cap too small
      rc = gx_rank_tables(G, S, tabs.data(), drop, pv.data(), pr.data(), cap, nOut.data(), &N);
    }
    printf("%d %" PRIu64 "\n", rc, rc ? (uint64_t)0 : N);
    if (!rc)
      for (int s = 0; s < S; s++) {
        printf("%zu\n", nOut[s]);
        for (size_t k = 0; k < nOut[s]; k++) printf("%" PRIu64 " %" PRIu64 "\n", ov[s][k], orr[s][k]);
      }
    printf("--\n");
  }
  fclose(f);
  // the argument checks: GX_ERR_ORDER
  const uint64_t one = 1;
  const gx_rank_table t{&one, &one, 1};
  size_t n = 0;
  uint64_t v = 0, r = 0;
  uint64_t* pv = &v;
  uint64_t* pr = &r;
  if (gx_rank_tables(0, 1, &t, 0, &pv, &pr, 1, &n, nullptr) != GX_ERR_ORDER) return 4;
  if (gx_rank_tables(1, 0, &t, 0, &pv, &pr, 1, &n, nullptr) != GX_ERR_ORDER) return 4;
  if (gx_rank_tables(1, 33, &t, 0, &pv, &pr, 1, &n, nullptr) != GX_ERR_ORDER) return 4;
  if (gx_rank_tables(1, 1, nullptr, 0, &pv, &pr, 1, &n, nullptr) != GX_ERR_ORDER) return 4;
  if (gx_rank_tables(1, 1, &t, 0, &pv, &pr, 1, nullptr, nullptr) != GX_ERR_ORDER) return 4;
  if (gx_rank_tables(1, 1, &t, 0, &pv, nullptr, 1, &n, nullptr) != GX_ERR_ORDER) return 4;
  if (gx_rank_tables(1, 1, &t, 0, &pv, &pr, 1, &n, nullptr) != GX_OK || n != 1 || v != 1 || r != 2) return 5;
  return 0;
}
