// Stand-alone driver of gx_kmer_revcomp / gx_kmer_stats / gx_format_kmers (genrich_amd/csrc/gx_emit.cpp) for tests/test_kmers.py,
// which compiles it together with gx_emit.cpp under -fsanitize=address,undefined and compares its output with
// tests/kmers_ref.py.  No device and no library: the C ABI entries gx_emit.cpp's other writers call are defined here and never
// reached.
//
// Spec file (argv[1]), per case:
//   "revcomp K N", then N codes.  Output: one line of the N answers (4294967295 where it is refused).
//   "table K FLANK REGIONS WP WG TOP NP NG", then NP pairs "code count" of the peaks and NG pairs of the genome (every other
//   count is 0).  Output: "refused <status>", or the table.
// Every case's output ends with "--\n".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static bool sparse(FILE* f, size_t n, std::vector<uint64_t>& table) {
  for (size_t i = 0; i < n; i++) {
    uint64_t code = 0, count = 0;
    if (fscanf(f, "%" SCNu64 " %" SCNu64, &code, &count) != 2 || code >= table.size()) return false;
    table[code] = count;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char kind[16];
  while (fscanf(f, "%15s", kind) == 1) {
    if (!strcmp(kind, "revcomp")) {
      int k = 0;
      size_t n = 0;
      if (fscanf(f, "%d %zu", &k, &n) != 2) return 2;
      for (size_t i = 0; i < n; i++) {
        uint32_t code = 0;
        if (fscanf(f, "%" SCNu32, &code) != 1) return 2;
        printf("%s%" PRIu32, i ? " " : "", gx_kmer_revcomp(k, code));
      }
      printf("\n--\n");
    } else if (!strcmp(kind, "table")) {
      int k = 0, flank = 0, top = 0;
      uint64_t regions = 0, wp = 0, wg = 0;
      size_t np = 0, ng = 0;
      if (fscanf(f, "%d %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %d %zu %zu", &k, &flank, &regions, &wp, &wg, &top, &np, &ng) != 8 || k < 1 || k > 12) return 2;
      // (exact-size heap arrays: a read or a write beyond them is the sanitizer's to catch)
      std::vector<uint64_t> cp((size_t)1 << (2 * k), 0), cg((size_t)1 << (2 * k), 0);
      if (!sparse(f, np, cp) || !sparse(f, ng, cg)) return 2;
      size_t n = 0;
      int rc = gx_kmer_stats(k, cp.data(), wp, cg.data(), wg, nullptr, 0, &n);
      std::vector<gx_kmer_row> rows(n);   // (exactly the rows there are)
      if (!rc) rc = gx_kmer_stats(k, cp.data(), wp, cg.data(), wg, rows.data(), n, nullptr);
      if (!rc) rc = gx_format_kmers(stdout, k, flank, regions, wp, wg, cp.data(), cg.data(), top);
      if (rc) printf("refused %d\n", rc);
      printf("--\n");
    } else {
      return 2;
    }
  }
  fclose(f);
  return 0;
}
