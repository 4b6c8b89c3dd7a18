// Stand-alone driver of gx_format_depth / gx_format_depth_metrics / gx_depth_metrics (genrich_amd/csrc/gx_emit.cpp) for
// tests/test_depth.py, which compiles it together with gx_emit.cpp under -fsanitize=address,undefined and compares its output
// with tests/depth_ref.py.  No device and no library: the C ABI entries gx_emit.cpp's other writers call are defined here and
// never reached.
//
// Spec file (argv[1]): per case one line "S", then per sample a line "rep is_ctrl total excluded zero min_v max_v k n", k lines
// "depth bases rsum rsq" (the non-empty classes) and n lines "v bases" (the deep list), all decimal.  Output (stdout): every
// case's distribution table, "--\n", its metrics table, "--\n".
#include <cinttypes>
#include <cmath>
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

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  for (;;) {
    int S = 0;
    if (fscanf(f, "%d", &S) != 1) break;
    // (exact-size heap arrays: a read beyond them is the sanitizer's to catch)
    std::vector<gx_depth_hist> hs((size_t)S);
    std::vector<std::vector<uint64_t>> arr((size_t)S * 5);
    for (int i = 0; i < S; i++) {
      gx_depth_hist& h = hs[(size_t)i];
      size_t k = 0, n = 0;
      if (fscanf(f, "%" SCNd32 " %" SCNd32 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %zu %zu", &h.rep, &h.is_ctrl, &h.total,
                 &h.excluded, &h.zero, &h.min_v, &h.max_v, &k, &n) != 9)
        return 2;
      std::vector<uint64_t>* a = &arr[(size_t)i * 5];
      for (int j = 0; j < 3; j++) a[j].assign(GX_DEPTH_BOUND, 0);
      for (size_t j = 0; j < k; j++) {
        uint64_t d = 0, b = 0, r = 0, q = 0;
        if (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &d, &b, &r, &q) != 4 || d >= GX_DEPTH_BOUND) return 2;
        a[0][d] = b;
        a[1][d] = r;
        a[2][d] = q;
      }
      a[3].resize(n);
      a[4].resize(n);
      for (size_t j = 0; j < n; j++)
        if (fscanf(f, "%" SCNu64 " %" SCNu64, &a[3][j], &a[4][j]) != 2) return 2;
      h.bases = a[0].data();
      h.rsum = a[1].data();
      h.rsq = a[2].data();
      h.deep_v = n ? a[3].data() : nullptr;
      h.deep_bases = n ? a[4].data() : nullptr;
      h.n_deep = n;
    }
    if (int rc = gx_format_depth(stdout, S, hs.data())) return 10 - rc;
    printf("--\n");
    if (int rc = gx_format_depth_metrics(stdout, S, hs.data())) return 10 - rc;
    printf("--\n");
  }
  fclose(f);
  // the ends of the domain: no base at all; one base at the largest pileup a sample can have
  std::vector<uint64_t> z(GX_DEPTH_BOUND, 0);
  gx_depth_hist h{};
  h.bases = h.rsum = h.rsq = z.data();
  gx_depth_metrics_t m;
  if (gx_depth_metrics(&h, &m) != GX_OK || m.bases != 0 || !std::isnan(m.mean) || !std::isnan(m.sd) || m.covered_fraction != 0.0 || m.median != 0) return 4;
  const uint64_t top = 0x7fffffffull, one = 1;
  h.total = 1;
  h.min_v = h.max_v = top;
  h.deep_v = &top;
  h.deep_bases = &one;
  h.n_deep = 1;
  if (gx_depth_metrics(&h, &m) != GX_OK || m.covered != 1 || m.sd != 0.0 || m.max_v != top || m.p99 != top / 120 || m.ge[6] != 1.0) return 4;
  // the argument checks: nothing written, GX_ERR_ORDER
  if (gx_depth_metrics(nullptr, &m) != GX_ERR_ORDER || gx_depth_metrics(&h, nullptr) != GX_ERR_ORDER) return 3;
  gx_depth_hist bad = h;
  bad.total = 2;                                        // covered + zero != B
  if (gx_depth_metrics(&bad, &m) != GX_ERR_ORDER) return 3;
  bad = h;
  bad.excluded = 2;                                     // excluded > total
  if (gx_depth_metrics(&bad, &m) != GX_ERR_ORDER) return 3;
  bad = h;
  bad.rsq = nullptr;                                    // a missing array
  if (gx_depth_metrics(&bad, &m) != GX_ERR_ORDER) return 3;
  bad = h;
  bad.deep_v = nullptr;                                 // a list without its values
  if (gx_depth_metrics(&bad, &m) != GX_ERR_ORDER) return 3;
  const uint64_t shallow = 120ull * GX_DEPTH_BOUND - 1;
  bad = h;
  bad.deep_v = &shallow;                                // a listed pileup below the bound
  if (gx_depth_metrics(&bad, &m) != GX_ERR_ORDER) return 3;
  bad = h;
  bad.min_v = 0;                                        // covered bases without a smallest pileup
  if (gx_depth_metrics(&bad, &m) != GX_ERR_ORDER) return 3;
  if (gx_format_depth(nullptr, 1, &h) != GX_ERR_ORDER || gx_format_depth(stdout, 0, &h) != GX_ERR_ORDER || gx_format_depth(stdout, 1, nullptr) != GX_ERR_ORDER) return 3;
  if (gx_format_depth(stdout, 1, &bad) != GX_ERR_ORDER || gx_format_depth_metrics(stdout, 1, &bad) != GX_ERR_ORDER) return 3;
  if (gx_format_depth_metrics(nullptr, 1, &h) != GX_ERR_ORDER || gx_format_depth_metrics(stdout, 0, &h) != GX_ERR_ORDER) return 3;
  return 0;
}
