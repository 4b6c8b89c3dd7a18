// Stand-alone driver of gx_saturation_overlap / gx_format_saturation / gx_saturation_thresholds (genrich_amd/csrc/gx_emit.cpp)
// for tests/test_saturation.py, which compiles it together with gx_emit.cpp under -fsanitize=address,undefined and compares its
// output with tests/saturation_ref.py and the golden text.  No device and no library: the C ABI entries gx_emit.cpp's other
// writers call are defined here and never reached.
//
// Spec file (argv[1]), a sequence of records:
//   "O nF nS", then nF + nS lines "chrom start end"                  -> a line "recovered in_run shared_bp"
//   "F nP n_full full_bp", then nP lines "threshold n_total n_kept n_peaks peak_bp genome_len status recovered in_run shared_bp"
//                                                                    -> the table, then "--\n"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
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

static bool read_peaks(FILE* f, std::vector<gx_peak>& v) {
  for (gx_peak& p : v) {
    p = gx_peak{};
    if (fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32, &p.chrom, &p.start, &p.end) != 3) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char what = 0;
  while (fscanf(f, " %c", &what) == 1) {
    if (what == 'O') {
      size_t nF = 0, nS = 0;
      if (fscanf(f, "%zu %zu", &nF, &nS) != 2) return 2;
      // (exact-size heap arrays: a read beyond them is the sanitizer's to catch)
      std::vector<gx_peak> full(nF), sub(nS);
      if (!read_peaks(f, full) || !read_peaks(f, sub)) return 2;
      uint64_t rec = 0, in = 0, bp = 0;
      if (int rc = gx_saturation_overlap(nF ? full.data() : nullptr, nF, nS ? sub.data() : nullptr, nS, &rec, &in, &bp)) return 10 - rc;
      printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", rec, in, bp);
    } else if (what == 'F') {
      int nP = 0;
      uint64_t nFull = 0, fullBp = 0;
      if (fscanf(f, "%d %" SCNu64 " %" SCNu64, &nP, &nFull, &fullBp) != 3 || nP < 1) return 2;
      std::vector<gx_sat_point> pts((size_t)nP);
      std::vector<uint64_t> rec((size_t)nP), in((size_t)nP), bp((size_t)nP);
      for (int j = 0; j < nP; j++) {
        gx_sat_point& p = pts[j];
        if (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd32 " %" SCNu64 " %" SCNu64 " %" SCNu64,
                   &p.threshold, &p.n_total, &p.n_kept, &p.n_peaks, &p.peak_bp, &p.genome_len, &p.status, &rec[j], &in[j], &bp[j]) != 10)
          return 2;
      }
      if (int rc = gx_format_saturation(stdout, nP, pts.data(), rec.data(), in.data(), bp.data(), nFull, fullBp)) return 10 - rc;
      printf("--\n");
    } else
      return 2;
  }
  fclose(f);
  // the thresholds at the ends of their domain
  uint64_t t[100];
  if (gx_saturation_thresholds(1, t) != GX_OK || t[0] != (uint64_t)1 << 32) return 4;
  if (gx_saturation_thresholds(100, t) != GX_OK || t[0] != 42949672 || t[99] != (uint64_t)1 << 32) return 4;
  if (gx_saturation_thresholds(0, t) != GX_ERR_ORDER || gx_saturation_thresholds(101, t) != GX_ERR_ORDER || gx_saturation_thresholds(3, nullptr) != GX_ERR_ORDER) return 4;
  // the argument checks: nothing written, GX_ERR_ORDER
  const gx_peak one{0, 10, 20, 0, 0.0f, 0.0f, 0.0f};
  const gx_sat_point pt{};
  const uint64_t z = 0;
  uint64_t a = 7;
  if (gx_saturation_overlap(nullptr, 1, &one, 1, &a, nullptr, nullptr) != GX_ERR_ORDER || a != 7) return 3;
  if (gx_saturation_overlap(&one, 1, nullptr, 1, &a, nullptr, nullptr) != GX_ERR_ORDER) return 3;
  if (gx_saturation_overlap(&one, 1, &one, 1, nullptr, nullptr, nullptr) != GX_OK) return 3;
  if (gx_saturation_overlap(nullptr, 0, nullptr, 0, &a, nullptr, nullptr) != GX_OK || a != 0) return 3;
  if (gx_format_saturation(nullptr, 1, &pt, &z, &z, &z, 0, 0) != GX_ERR_ORDER) return 3;
  if (gx_format_saturation(stdout, 0, &pt, &z, &z, &z, 0, 0) != GX_ERR_ORDER) return 3;
  if (gx_format_saturation(stdout, 1, nullptr, &z, &z, &z, 0, 0) != GX_ERR_ORDER) return 3;
  if (gx_format_saturation(stdout, 1, &pt, &z, nullptr, &z, 0, 0) != GX_ERR_ORDER) return 3;
  return 0;
}
