// Stand-alone driver of gx_format_peak_signal (genrich_amd/csrc/gx_emit.cpp) for tests/test_peak_signal.py, which compiles it
// together with gx_emit.cpp under -fsanitize=address,undefined and compares its output with tests/peaksig_ref.py.  No device
// and no library: the C ABI entries gx_emit.cpp's other writers call are defined here and never reached.
//
// Spec file (argv[1]): per case one line "C P S" (chromosome names, peaks, samples), C names, P lines "chrom start end", then
// per sample a line "rep is_ctrl" and P lines "area max summit covered at_summit", all decimal.  Output (stdout): every case's
// table, then "--\n".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
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
  for (;;) {
    size_t C = 0, P = 0;
    int S = 0;
    if (fscanf(f, "%zu %zu %d", &C, &P, &S) != 3) break;
    // (exact-size heap arrays: a read beyond them is the sanitizer's to catch)
    std::vector<std::string> nameStr(C);
    std::vector<const char*> names(C);
    for (size_t i = 0; i < C; i++) {
      char buf[128];
      if (fscanf(f, "%127s", buf) != 1) return 2;
      nameStr[i] = buf;
    }
    for (size_t i = 0; i < C; i++) names[i] = nameStr[i].c_str();
    std::vector<gx_region> pk(P);
    for (size_t k = 0; k < P; k++)
      if (fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32, &pk[k].chrom, &pk[k].start, &pk[k].end) != 3 || pk[k].chrom >= C) return 2;
    std::vector<int> rep((size_t)S), ctrl((size_t)S);
    std::vector<std::vector<int64_t>> area((size_t)S), mx((size_t)S), at((size_t)S);
    std::vector<std::vector<uint32_t>> sm((size_t)S), cov((size_t)S);
    std::vector<const int64_t*> pa((size_t)S), pm((size_t)S), pt((size_t)S);
    std::vector<const uint32_t*> ps((size_t)S), pc((size_t)S);
    for (int i = 0; i < S; i++) {
      if (fscanf(f, "%d %d", &rep[i], &ctrl[i]) != 2) return 2;
      area[i].resize(P); mx[i].resize(P); at[i].resize(P); sm[i].resize(P); cov[i].resize(P);
      for (size_t k = 0; k < P; k++)
        if (fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNu32 " %" SCNu32 " %" SCNd64, &area[i][k], &mx[i][k], &sm[i][k], &cov[i][k], &at[i][k]) != 5) return 2;
      pa[i] = area[i].data(); pm[i] = mx[i].data(); pt[i] = at[i].data(); ps[i] = sm[i].data(); pc[i] = cov[i].data();
    }
    if (int rc = gx_format_peak_signal(stdout, names.data(), pk.data(), P, S, rep.data(), ctrl.data(), pa.data(), pm.data(), ps.data(), pc.data(),
                                       pt.data()))
      return 10 - rc;
    printf("--\n");
  }
  fclose(f);
  // the argument checks: nothing written, GX_ERR_ORDER; no peak and no sample are legal without any array
  const char* nm[1] = {"chrA"};
  const gx_region one{0, 1, 2};
  const int zero = 0;
  const int64_t v = 0;
  const uint32_t u = 0;
  const int64_t* pv[1] = {&v};
  const uint32_t* pu[1] = {&u};
  const int64_t* none[1] = {nullptr};
  if (gx_format_peak_signal(nullptr, nm, &one, 1, 1, &zero, &zero, pv, pv, pu, pu, pv) != GX_ERR_ORDER) return 3;
  if (gx_format_peak_signal(stdout, nm, nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != GX_ERR_ORDER) return 3;
  if (gx_format_peak_signal(stdout, nm, &one, 1, 1, nullptr, &zero, pv, pv, pu, pu, pv) != GX_ERR_ORDER) return 3;
  if (gx_format_peak_signal(stdout, nm, &one, 1, 1, &zero, &zero, pv, none, pu, pu, pv) != GX_ERR_ORDER) return 3;
  if (gx_format_peak_signal(stdout, nm, &one, 1, -1, &zero, &zero, pv, pv, pu, pu, pv) != GX_ERR_ORDER) return 3;
  if (gx_format_peak_signal(stdout, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != GX_OK) return 4;
  return 0;
}
