// Stand-alone driver of gx_format_correlation (genrich_amd/csrc/gx_emit.cpp) for tests/test_gram.py, which compiles it together
// with gx_emit.cpp under -fsanitize=address,undefined and compares its output with tests/gram_ref.py.  No device and no
// library: the C ABI entries gx_emit.cpp's other writers call are defined here and never reached.
//
// Spec file (argv[1]): per case one line "S n n_zero skip_zeros", then S lines "name sum_hi sum_lo" and S * S lines
// "gram_hi gram_lo" (row-major; hexadecimal words).  Output (stdout): every case's text, each followed by "--\n".
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
    int S = 0, skip = 0;
    uint64_t n = 0, nz = 0;
    if (fscanf(f, "%d %" SCNu64 " %" SCNu64 " %d", &S, &n, &nz, &skip) != 4) break;
    std::vector<std::string> names((size_t)S);
    // (exact-size heap arrays: a read beyond them is the sanitizer's to catch)
    std::vector<gx_u128> sum((size_t)S), gram((size_t)S * S);
    char name[256];
    for (int i = 0; i < S; i++) {
      if (fscanf(f, "%255s %" SCNx64 " %" SCNx64, name, &sum[i].hi, &sum[i].lo) != 3) return 2;
      names[i] = name;
    }
    for (size_t k = 0; k < (size_t)S * S; k++)
      if (fscanf(f, "%" SCNx64 " %" SCNx64, &gram[k].hi, &gram[k].lo) != 2) return 2;
    std::vector<const char*> np;
    for (const std::string& s : names) np.push_back(s.c_str());
    if (int rc = gx_format_correlation(stdout, S, np.data(), n, nz, sum.data(), gram.data(), skip)) return 10 - rc;
    printf("--\n");
  }
  fclose(f);
  // the argument checks: nothing written, GX_ERR_ORDER
  const gx_u128 one{1, 0};
  const char* nm = "x";
  if (gx_format_correlation(stdout, 0, &nm, 1, 0, &one, &one, 0) != GX_ERR_ORDER) return 3;
  if (gx_format_correlation(stdout, 1, nullptr, 1, 0, &one, &one, 0) != GX_ERR_ORDER) return 3;
  if (gx_format_correlation(stdout, 1, &nm, 1, 0, nullptr, &one, 0) != GX_ERR_ORDER) return 3;
  if (gx_format_correlation(stdout, 1, &nm, 1, 0, &one, nullptr, 0) != GX_ERR_ORDER) return 3;
  if (gx_format_correlation(stdout, 1, &nm, 1, 2, &one, &one, 1) != GX_ERR_ORDER) return 3;   // n_zero > n
  if (gx_format_correlation(nullptr, 1, &nm, 1, 0, &one, &one, 0) != GX_ERR_ORDER) return 3;
  return 0;
}
