// Stand-alone driver of gx_gc_metrics / gx_format_gc_bias / gx_format_gc_peaks / gx_gc_class (genrich_amd/csrc/gx_emit.cpp) for
// tests/test_gcbias.py, which compiles it together with gx_emit.cpp under -fsanitize=address,undefined and compares its output
// with tests/gcbias_ref.py.  No device and no library: the C ABI entries gx_emit.cpp's other writers call are defined here and
// never reached.
//
// Spec file (argv[1]): per case one line "bias S W", then per sample a line "rep is_ctrl f_unclassed n_unclassed w_unclassed" and
// three lines of W + 1 numbers (F, Nn, Nw); or one line "peaks N" and N lines "chrom start end gc acgt" (the names are chr0 ..
// chr9).  Output (stdout): every case's table, then "--\n".
#include <cinttypes>
#include <cmath>
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

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  const char* names[10] = {"chr0", "chr1", "chr2", "chr3", "chr4", "chr5", "chr6", "chr7", "chr8", "chr9"};
  char kind[16];
  while (fscanf(f, "%15s", kind) == 1) {
    if (!strcmp(kind, "bias")) {
      int S = 0, W = 0;
      if (fscanf(f, "%d %d", &S, &W) != 2 || S < 1 || W < 1 || W > GX_GC_MAX_WINDOW) return 2;
      // (exact-size heap arrays: a read beyond them is the sanitizer's to catch)
      std::vector<int> rep((size_t)S), ctrl((size_t)S);
      std::vector<uint64_t> fu((size_t)S), nu((size_t)S), wu((size_t)S);
      std::vector<std::vector<uint64_t>> rows((size_t)S * 3);
      std::vector<const uint64_t*> pF, pN, pW;
      for (int i = 0; i < S; i++) {
        if (fscanf(f, "%d %d %" SCNu64 " %" SCNu64 " %" SCNu64, &rep[(size_t)i], &ctrl[(size_t)i], &fu[(size_t)i], &nu[(size_t)i], &wu[(size_t)i]) != 5) return 2;
        for (int k = 0; k < 3; k++) {
          std::vector<uint64_t>& r = rows[(size_t)i * 3 + (size_t)k];
          r.resize((size_t)W + 1);
          for (uint64_t& v : r)
            if (fscanf(f, "%" SCNu64, &v) != 1) return 2;
        }
        pF.push_back(rows[(size_t)i * 3].data());
        pN.push_back(rows[(size_t)i * 3 + 1].data());
        pW.push_back(rows[(size_t)i * 3 + 2].data());
      }
      if (int rc = gx_format_gc_bias(stdout, S, rep.data(), ctrl.data(), W, pF.data(), fu.data(), pN.data(), pW.data(), nu.data(), wu.data())) return 10 - rc;
    } else if (!strcmp(kind, "peaks")) {
      size_t N = 0;
      if (fscanf(f, "%zu", &N) != 1) return 2;
      std::vector<gx_region> reg(N);
      std::vector<uint64_t> gc(N), acgt(N);
      for (size_t i = 0; i < N; i++)
        if (fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64, &reg[i].chrom, &reg[i].start, &reg[i].end, &gc[i], &acgt[i]) != 5 || reg[i].chrom > 9)
          return 2;
      if (int rc = gx_format_gc_peaks(stdout, names, reg.data(), N, gc.data(), acgt.data())) return 10 - rc;
    } else {
      return 2;
    }
    printf("--\n");
  }
  fclose(f);
  // the class fold at its ends and ties
  if (gx_gc_class(200, 0) != 0 || gx_gc_class(200, 1) != 1 || gx_gc_class(200, 200) != 100 || gx_gc_class(1, 0) != 0 || gx_gc_class(1, 1) != 100 ||
      gx_gc_class(4096, 4096) != 100 || gx_gc_class(4096, 20) != 0 || gx_gc_class(4096, 21) != 1 || gx_gc_class(3, 4) != -1 || gx_gc_class(0, 0) != -1 ||
      gx_gc_class(4097, 1) != -1)
    return 4;
  // the widest window with the largest counts; a sample without intervals; a genome without classed windows
  gx_gc_metrics_t m;
  {
    const int W = GX_GC_MAX_WINDOW;
    std::vector<uint64_t> F((size_t)W + 1), Nn((size_t)W + 1), Nw((size_t)W + 1), zero((size_t)W + 1, 0);
    for (int g = 0; g <= W; g++) {
      F[(size_t)g] = (1ull << 25) + 3 * (uint64_t)g;
      Nn[(size_t)g] = (1ull << 18) + (uint64_t)g;
      Nw[(size_t)g] = 120 * Nn[(size_t)g] - (uint64_t)(g % 7);
    }
    if (gx_gc_metrics(W, F.data(), 5, Nn.data(), Nw.data(), 7, 9, &m) != GX_OK || m.windows_unclassed != 5 || !(m.ratio[50] > 0.0) || m.ratio_min_class < 0) return 4;
    if (gx_gc_metrics(W, F.data(), 0, zero.data(), zero.data(), 0, 0, &m) != GX_OK || !std::isnan(m.ratio[50]) || !std::isnan(m.mean_gc_sample) ||
        m.ratio_min_class != -1 || !(m.mean_gc_genome > 0.0))
      return 4;
    if (gx_gc_metrics(W, zero.data(), 0, Nn.data(), Nw.data(), 0, 0, &m) != GX_OK || !std::isnan(m.ratio[0]) || !std::isnan(m.mean_gc_genome) || m.ratio_max_class != -1)
      return 4;
  }
  // the argument checks: nothing written, GX_ERR_ORDER
  const uint64_t a2[2] = {3, 4}, n2[2] = {1, 1}, w2[2] = {120, 60}, light[2] = {120, 0}, heavy[2] = {121, 60};
  if (gx_gc_metrics(1, a2, 0, n2, w2, 0, 0, nullptr) != GX_ERR_ORDER || gx_gc_metrics(1, nullptr, 0, n2, w2, 0, 0, &m) != GX_ERR_ORDER) return 3;
  if (gx_gc_metrics(0, a2, 0, n2, w2, 0, 0, &m) != GX_ERR_ORDER || gx_gc_metrics(GX_GC_MAX_WINDOW + 1, a2, 0, n2, w2, 0, 0, &m) != GX_ERR_ORDER) return 3;
  if (gx_gc_metrics(1, a2, 0, n2, light, 0, 0, &m) != GX_ERR_ORDER || gx_gc_metrics(1, a2, 0, n2, heavy, 0, 0, &m) != GX_ERR_ORDER) return 3;   // a weight outside [n, 120 n]
  const int r0 = 0;
  const uint64_t z = 0;
  const uint64_t *pa = a2, *pn = n2, *pw = w2, *ph = heavy;
  if (gx_format_gc_bias(nullptr, 1, &r0, &r0, 1, &pa, &z, &pn, &pw, &z, &z) != GX_ERR_ORDER || gx_format_gc_bias(stdout, 0, &r0, &r0, 1, &pa, &z, &pn, &pw, &z, &z) != GX_ERR_ORDER ||
      gx_format_gc_bias(stdout, 1, &r0, &r0, 1, &pa, &z, &pn, &ph, &z, &z) != GX_ERR_ORDER || gx_format_gc_bias(stdout, 1, &r0, &r0, 1, &pa, nullptr, &pn, &pw, &z, &z) != GX_ERR_ORDER)
    return 3;
  const gx_region one = {0, 10, 20};
  const uint64_t g5 = 5, a4 = 4, a11 = 11;
  if (gx_format_gc_peaks(nullptr, names, &one, 1, &g5, &a11) != GX_ERR_ORDER || gx_format_gc_peaks(stdout, names, &one, 1, &g5, &a4) != GX_ERR_ORDER ||   // gc > acgt
      gx_format_gc_peaks(stdout, names, &one, 1, &g5, &a11) != GX_ERR_ORDER || gx_format_gc_peaks(stdout, names, nullptr, 1, &g5, &a11) != GX_ERR_ORDER)  // acgt > length
    return 3;
  return 0;
}
