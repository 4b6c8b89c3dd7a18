// Stand-alone driver of gx_format_summits (genrich_amd/csrc/gx_emit.cpp) for tests/test_summits.py, which compiles it together
// with gx_emit.cpp under -fsanitize=address,undefined and compares its output with tests/summits_ref.py.  No device and no
// library: the C ABI entries gx_emit.cpp's other writers call are defined here and never reached.
//
// Spec file (argv[1]): per case one line "C P N" (chromosome names, peaks, summits), C names, P lines "chrom start end", N lines
// "peak pos width height prominence", all decimal.  Output (stdout): every case's table, then "--\n".
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
    size_t C = 0, P = 0, N = 0;
    if (fscanf(f, "%zu %zu %zu", &C, &P, &N) != 3) break;
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
    std::vector<gx_summit> sm(N);
    for (size_t i = 0; i < N; i++) {
      sm[i].pad = 0;
      if (fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNd64 " %" SCNd64, &sm[i].peak, &sm[i].pos, &sm[i].width, &sm[i].height120,
                 &sm[i].prominence120) != 5)
        return 2;
    }
    if (int rc = gx_format_summits(stdout, names.data(), pk.data(), P, sm.data(), N)) return 10 - rc;
    printf("--\n");
  }
  fclose(f);
  // the argument checks: nothing written, GX_ERR_ORDER; no summit is legal without any array
  const char* nm[1] = {"chrA"};
  const gx_region one{0, 10, 20};
  const gx_summit ok{0, 4, 3, 0, 120, 60}, other{0, 4, 1, 0, 120, 60}, beyond{1, 0, 1, 0, 1, 1}, wide{0, 9, 3, 0, 1, 1}, empty{0, 4, 0, 0, 1, 1},
      before{0, 0, 3, 0, 1, 1};
  const gx_summit twice[2] = {ok, other};
  if (gx_format_summits(nullptr, nm, &one, 1, &ok, 1) != GX_ERR_ORDER) return 3;
  if (gx_format_summits(stdout, nm, nullptr, 1, &ok, 1) != GX_ERR_ORDER) return 3;
  if (gx_format_summits(stdout, nm, &one, 1, nullptr, 1) != GX_ERR_ORDER) return 3;
  if (gx_format_summits(stdout, nm, &one, 1, &beyond, 1) != GX_ERR_ORDER) return 3;   // a peak the list does not have
  if (gx_format_summits(stdout, nm, &one, 1, &wide, 1) != GX_ERR_ORDER) return 3;     // a plateau beyond its peak's end
  if (gx_format_summits(stdout, nm, &one, 1, &empty, 1) != GX_ERR_ORDER) return 3;
  if (gx_format_summits(stdout, nm, &one, 1, &before, 1) != GX_ERR_ORDER) return 3;   // ... before its start
  if (gx_format_summits(stdout, nm, &one, 1, twice, 2) != GX_ERR_ORDER) return 3;     // not ascending
  if (gx_format_summits(stdout, nullptr, nullptr, 0, nullptr, 0) != GX_OK) return 4;
  return 0;
}
