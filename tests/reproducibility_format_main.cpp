// Stand-alone driver of gx_peaks_supported / gx_reproducibility_figures / gx_format_reproducibility /
// gx_format_reproducibility_metrics / gx_format_narrowpeak (genrich_amd/csrc/gx_emit.cpp) for tests/test_reproducibility.py, which
// compiles it together with gx_emit.cpp under -fsanitize=address,undefined and compares its output with
// tests/reproducibility_ref.py and the golden text.  No device and no library: the C ABI entries gx_emit.cpp's other writers
// call are defined here and never reached.
//
// Spec file (argv[1]), a sequence of records:
//   "S nA nB pct", then nA + nB lines "chrom start end"                -> a line of nA digits, hit[i]
//   "G nRun R pct seed run_bp", then nRun lines "chrom start end", then per call (3 R + 2, the library's order) a line
//   "n_events n_peaks peak_bp status" and n_peaks lines "chrom start end"
//                                                                      -> the call table, "--\n", the metrics, "--\n", a line of
//                                                                         nRun digits for the conservative set, one for the optimal
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

static void put_bits(const std::vector<uint8_t>& v) {
  for (uint8_t b : v) putchar(b ? '1' : '0');
  putchar('\n');
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char what = 0;
  while (fscanf(f, " %c", &what) == 1) {
    if (what == 'S') {
      size_t nA = 0, nB = 0;
      int pct = 0;
      if (fscanf(f, "%zu %zu %d", &nA, &nB, &pct) != 3) return 2;
      // (exact-size heap arrays: a read or a write beyond them is the sanitizer's to catch)
      std::vector<gx_peak> a(nA), b(nB);
      std::vector<uint8_t> hit(nA);
      if (!read_peaks(f, a) || !read_peaks(f, b)) return 2;
      if (int rc = gx_peaks_supported(nA ? a.data() : nullptr, nA, nB ? b.data() : nullptr, nB, pct, nA ? hit.data() : nullptr)) return 10 - rc;
      put_bits(hit);
    } else if (what == 'G') {
      size_t nRun = 0;
      int R = 0, pct = 0;
      uint64_t seed = 0, runBp = 0;
      if (fscanf(f, "%zu %d %d %" SCNu64 " %" SCNu64, &nRun, &R, &pct, &seed, &runBp) != 5 || R < 1) return 2;
      std::vector<gx_peak> run(nRun);
      if (!read_peaks(f, run)) return 2;
      const size_t nC = 3 * (size_t)R + 2;
      std::vector<gx_repro_call> calls(nC);
      std::vector<std::vector<gx_peak>> lists(nC);
      std::vector<const gx_peak*> ptrs(nC);
      for (size_t i = 0; i < nC; i++) {
        gx_repro_call& c = calls[i];
        c.kind = i < (size_t)R ? GX_REPRO_ALONE : i < 3 * (size_t)R ? GX_REPRO_SELF : GX_REPRO_POOLED;
        c.rep = i < (size_t)R ? (int)i : i < 3 * (size_t)R ? (int)(i - R) / 2 : -1;
        c.half = i < (size_t)R ? -1 : i < 3 * (size_t)R ? (int)(i - R) % 2 : (int)(i - 3 * R);
        if (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd32, &c.n_events, &c.n_peaks, &c.peak_bp, &c.status) != 4) return 2;
        lists[i].resize((size_t)c.n_peaks);
        if (!read_peaks(f, lists[i])) return 2;
        ptrs[i] = lists[i].empty() ? nullptr : lists[i].data();
      }
      gx_repro_figures fig;
      std::vector<uint64_t> pairs((size_t)R * (R - 1) / 2), self((size_t)R), inRun(nC), runSup(nC);
      std::vector<uint8_t> cons(nRun), opt(nRun);
      if (int rc = gx_reproducibility_figures(nRun ? run.data() : nullptr, nRun, R, calls.data(), ptrs.data(), pct, &fig,
                                              pairs.empty() ? nullptr : pairs.data(), self.data(), inRun.data(), runSup.data(),
                                              nRun ? cons.data() : nullptr, nRun ? opt.data() : nullptr))
        return 10 - rc;
      if (int rc = gx_format_reproducibility(stdout, R, calls.data(), inRun.data(), runSup.data(), nRun, runBp, pct, seed)) return 10 - rc;
      printf("--\n");
      if (int rc = gx_format_reproducibility_metrics(stdout, &fig, pairs.empty() ? nullptr : pairs.data(), self.data())) return 10 - rc;
      printf("--\n");
      put_bits(cons);
      put_bits(opt);
    } else
      return 2;
  }
  fclose(f);
  // the argument checks: nothing written, GX_ERR_ORDER
  const gx_peak one{0, 10, 20, 0, 0.0f, 0.0f, 0.0f};
  uint8_t h = 7;
  if (gx_peaks_supported(&one, 1, &one, 1, 101, &h) != GX_ERR_ORDER || gx_peaks_supported(&one, 1, &one, 1, -1, &h) != GX_ERR_ORDER || h != 7) return 3;
  if (gx_peaks_supported(nullptr, 1, &one, 1, 50, &h) != GX_ERR_ORDER || gx_peaks_supported(&one, 1, nullptr, 1, 50, &h) != GX_ERR_ORDER) return 3;
  if (gx_peaks_supported(&one, 1, &one, 1, 50, nullptr) != GX_ERR_ORDER) return 3;
  if (gx_peaks_supported(&one, 1, &one, 1, 100, &h) != GX_OK || h != 1) return 3;
  if (gx_peaks_supported(nullptr, 0, nullptr, 0, 50, nullptr) != GX_OK) return 3;
  // a list of calls in another order than the library's is refused
  gx_repro_call five[5] = {{GX_REPRO_ALONE, 0, -1, 0, 0, 0, 0}, {GX_REPRO_SELF, 0, 0, 0, 0, 0, 0}, {GX_REPRO_SELF, 0, 1, 0, 0, 0, 0},
                           {GX_REPRO_POOLED, -1, 0, 0, 0, 0, 0}, {GX_REPRO_POOLED, -1, 1, 0, 0, 0, 0}};
  const gx_peak* none[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  gx_repro_figures fig;
  uint64_t self1 = 9, in5[5], sup5[5];
  if (gx_reproducibility_figures(nullptr, 0, 1, five, none, 50, &fig, nullptr, &self1, in5, sup5, nullptr, nullptr) != GX_OK || self1 != 0 ||
      fig.verdict != GX_REPRO_NA)
    return 5;
  five[1].half = 1;
  if (gx_reproducibility_figures(nullptr, 0, 1, five, none, 50, &fig, nullptr, &self1, in5, sup5, nullptr, nullptr) != GX_ERR_ORDER) return 5;
  five[1].half = 0;
  if (gx_reproducibility_figures(nullptr, 0, 0, five, none, 50, &fig, nullptr, &self1, in5, sup5, nullptr, nullptr) != GX_ERR_ORDER) return 5;
  if (gx_reproducibility_figures(nullptr, 0, 1, five, none, 101, &fig, nullptr, &self1, in5, sup5, nullptr, nullptr) != GX_ERR_ORDER) return 5;
  if (gx_format_reproducibility(nullptr, 1, five, in5, sup5, 0, 0, 50, 1) != GX_ERR_ORDER) return 5;
  if (gx_format_reproducibility_metrics(stdout, nullptr, nullptr, &self1) != GX_ERR_ORDER) return 5;
  // the list writer: a peak's name is its index behind first_index
  const char* names[1] = {"chrA"};
  const gx_peak two[2] = {{0, 10, 20, 15, 30.0f, 2.0f, GX_SKIP}, {0, 40, 90, 60, 100.0f, 3.0f, 1.5f}};
  if (gx_format_narrowpeak(two, 2, names, 7, stdout) != GX_OK) return 6;
  if (gx_format_narrowpeak(nullptr, 1, names, 0, stdout) != GX_ERR_ORDER || gx_format_narrowpeak(nullptr, 0, nullptr, 0, stdout) != GX_OK) return 6;
  return 0;
}
