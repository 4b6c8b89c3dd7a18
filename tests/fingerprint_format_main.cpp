// Stand-alone driver of gx_format_fingerprint / gx_format_fingerprint_metrics (genrich_amd/csrc/gx_emit.cpp) for
// tests/test_fingerprint.py, which compiles it together with gx_emit.cpp under -fsanitize=address,undefined and compares its
// output with tests/fingerprint_ref.py.  No device and no library: the C ABI entries gx_emit.cpp's other writers call are
// defined here and never reached.
//
// Spec file (argv[1]): per case one line "S", then per sample a line "name ctrl_of m" and m lines "class count sum" (its
// non-empty classes; decimal).  Output (stdout): every case's curve table, "--\n", its metrics table, "--\n".
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
    int S = 0;
    if (fscanf(f, "%d", &S) != 1) break;
    std::vector<std::string> names((size_t)S);
    // (exact-size heap arrays: a read beyond them is the sanitizer's to catch)
    std::vector<uint64_t> count((size_t)S * GX_FP_NC, 0), sum((size_t)S * GX_FP_NC, 0);
    std::vector<int> ctrl((size_t)S);
    char name[256];
    for (int i = 0; i < S; i++) {
      int m = 0;
      if (fscanf(f, "%255s %d %d", name, &ctrl[i], &m) != 3) return 2;
      names[i] = name;
      for (int j = 0; j < m; j++) {
        int k = 0;
        uint64_t c = 0, s = 0;
        if (fscanf(f, "%d %" SCNu64 " %" SCNu64, &k, &c, &s) != 3 || k < 0 || k >= GX_FP_NC) return 2;
        count[(size_t)i * GX_FP_NC + k] = c;
        sum[(size_t)i * GX_FP_NC + k] = s;
      }
    }
    std::vector<const char*> np;
    for (const std::string& s : names) np.push_back(s.c_str());
    if (int rc = gx_format_fingerprint(stdout, S, np.data(), count.data(), sum.data())) return 10 - rc;
    printf("--\n");
    if (int rc = gx_format_fingerprint_metrics(stdout, S, np.data(), count.data(), sum.data(), ctrl.data())) return 10 - rc;
    printf("--\n");
  }
  fclose(f);
  // the classes at the ends of the domain
  if (gx_fp_class(0) != 0 || gx_fp_class(UINT64_MAX) != GX_FP_NC - 1 || gx_fp_class_hi(GX_FP_NC - 1) != UINT64_MAX) return 4;
  // the argument checks: nothing written, GX_ERR_ORDER
  std::vector<uint64_t> one((size_t)GX_FP_NC, 1);
  const char* nm = "x";
  const int self = 0, beyond = 1;
  if (gx_format_fingerprint(stdout, 0, &nm, one.data(), one.data()) != GX_ERR_ORDER) return 3;
  if (gx_format_fingerprint(stdout, 1, nullptr, one.data(), one.data()) != GX_ERR_ORDER) return 3;
  if (gx_format_fingerprint(stdout, 1, &nm, nullptr, one.data()) != GX_ERR_ORDER) return 3;
  if (gx_format_fingerprint(stdout, 1, &nm, one.data(), nullptr) != GX_ERR_ORDER) return 3;
  if (gx_format_fingerprint(nullptr, 1, &nm, one.data(), one.data()) != GX_ERR_ORDER) return 3;
  if (gx_format_fingerprint_metrics(stdout, 1, &nm, one.data(), one.data(), &self) != GX_ERR_ORDER) return 3;     // its own control
  if (gx_format_fingerprint_metrics(stdout, 1, &nm, one.data(), one.data(), &beyond) != GX_ERR_ORDER) return 3;   // no such sample
  if (gx_format_fingerprint_metrics(nullptr, 1, &nm, one.data(), one.data(), nullptr) != GX_ERR_ORDER) return 3;
  return 0;
}
