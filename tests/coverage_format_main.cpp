// Stand-alone driver of gx_format_coverage / gx_write_coverage (genrich_amd/csrc/gx_emit.cpp) for tests/test_coverage.py, which
// compiles it together with gx_emit.cpp under -fsanitize=address,undefined and compares its output with tests/coverage_ref.py.
// No device and no library: the C ABI entries gx_emit.cpp calls are defined here -- the coverage ones serve the arrays of the
// spec file, the others are never reached.
//
// Spec file (argv[1]): one line per chromosome, "name len bin_size scale n_bins sum_0 ... sum_{n-1}".  Output (stdout): every
// line's gx_format_coverage text, then "--\n", then gx_write_coverage over all of them as one sample (the first line's scale).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/genrich_amd.h"

namespace {
struct Row {
  std::string name;
  uint32_t len = 0, W = 0;
  double scale = 1.0;
  std::vector<int64_t> sums;
};
std::vector<Row> rows;
}  // namespace

struct gx_ctx { int unused; };

extern "C" {
int gx_peak_count(gx_ctx*, size_t*) { return GX_ERR_ORDER; }
int gx_get_peaks(gx_ctx*, gx_peak*, size_t) { return GX_ERR_ORDER; }
int gx_get_peak_counts(gx_ctx*, int, int*, int*, int64_t*, size_t, int64_t*, int64_t*) { return GX_ERR_ORDER; }
int gx_get_region_counts(gx_ctx*, int, int*, int*, int64_t*, size_t, int64_t*, int64_t*) { return GX_ERR_ORDER; }
int gx_interval_count(gx_ctx*, int, int, size_t*) { return GX_ERR_ORDER; }
int gx_get_intervals(gx_ctx*, int, int, size_t, uint32_t*, float*, float*, float*, float*) { return GX_ERR_ORDER; }
int gx_coverage_bin_count(gx_ctx*, int chrom, size_t* n) {
  *n = rows[chrom].sums.size();
  return GX_OK;
}
int gx_coverage_layout(gx_ctx*, int chrom, uint32_t* W, uint32_t* len) {
  if (W) *W = rows[chrom].W;
  if (len) *len = rows[chrom].len;
  return GX_OK;
}
int gx_get_coverage(gx_ctx*, int, int chrom, int*, int*, int64_t* out, size_t cap) {
  // (a fresh exact-size copy: a read or write beyond `cap` is the sanitizer's to catch)
  std::vector<int64_t> copy(rows[chrom].sums.begin(), rows[chrom].sums.begin() + cap);
  if (cap) memcpy(out, copy.data(), cap * sizeof(int64_t));
  return GX_OK;
}
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char name[256];
  for (;;) {
    Row r;
    unsigned long n = 0;
    if (fscanf(f, "%255s %u %u %lf %lu", name, &r.len, &r.W, &r.scale, &n) != 5) break;
    r.name = name;
    r.sums.resize(n);
    for (unsigned long i = 0; i < n; i++) {
      long long v = 0;
      if (fscanf(f, "%lld", &v) != 1) return 2;
      r.sums[i] = v;
    }
    rows.push_back(std::move(r));
  }
  fclose(f);
  for (const Row& r : rows) {
    // (exact-size heap copy, as above)
    std::vector<int64_t> copy(r.sums);
    copy.shrink_to_fit();
    if (int rc = gx_format_coverage(stdout, r.name.c_str(), r.len, r.W, copy.data(), copy.size(), r.scale)) return 10 - rc;
  }
  printf("--\n");
  std::vector<const char*> names;
  for (const Row& r : rows) names.push_back(r.name.c_str());
  gx_ctx ctx{0};
  if (int rc = gx_write_coverage(&ctx, 0, names.data(), (int)names.size(), rows.empty() ? 1.0 : rows[0].scale, stdout)) return 10 - rc;
  // the argument checks: nothing written, GX_ERR_ORDER
  const int64_t one = 120;
  if (gx_format_coverage(stdout, "x", 10, 0, &one, 1, 1.0) != GX_ERR_ORDER) return 3;
  if (gx_format_coverage(stdout, "x", 10, 5, &one, 1, 1.0) != GX_ERR_ORDER) return 3;
  if (gx_format_coverage(stdout, nullptr, 10, 10, &one, 1, 1.0) != GX_ERR_ORDER) return 3;
  return 0;
}
