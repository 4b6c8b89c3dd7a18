// Stand-alone driver of gx_format_profile / gx_format_profile_rows (genrich_amd/csrc/gx_emit.cpp) for tests/test_profile.py,
// which compiles it together with gx_emit.cpp under -fsanitize=address,undefined and compares its output with
// tests/profile_ref.py.  No device and no library: the C ABI entries gx_emit.cpp calls are defined here and never reached.
//
// Spec file (argv[1]), whitespace-separated:
//   flank bin_size n_counted n_samples n_bins
//   n_samples lines:  sample_name agg_0 ... agg_{n_bins-1}
//   n_names name_0 ... name_{n_names-1}                    (chromosome names, by index)
//   n_anchors first n_rows
//   n_anchors lines:  chrom start end row_name|* strand    (* = no name)
//   n_rows lines:     cell_0 ... cell_{n_bins-1}
// Output (stdout): gx_format_profile's table, "--\n", gx_format_profile_rows' rows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

namespace {
bool read_row(FILE* f, std::vector<int64_t>& row, size_t n) {
  row.resize(n);
  row.shrink_to_fit();   // (exact-size heap arrays: a read beyond them is the sanitizer's to catch)
  for (size_t i = 0; i < n; i++) {
    long long v = 0;
    if (fscanf(f, "%lld", &v) != 1) return false;
    row[i] = v;
  }
  return true;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  unsigned F = 0, B = 0, nb = 0;
  unsigned long counted = 0, nS = 0, nNames = 0, nA = 0, first = 0, nRows = 0;
  char word[256];
  if (fscanf(f, "%u %u %lu %lu %u", &F, &B, &counted, &nS, &nb) != 5) return 2;
  std::vector<std::string> sampleNames(nS);
  std::vector<std::vector<int64_t>> aggs(nS);
  for (unsigned long s = 0; s < nS; s++) {
    if (fscanf(f, "%255s", word) != 1) return 2;
    sampleNames[s] = word;
    if (!read_row(f, aggs[s], nb)) return 2;
  }
  if (fscanf(f, "%lu", &nNames) != 1) return 2;
  std::vector<std::string> names(nNames);
  for (auto& n : names) {
    if (fscanf(f, "%255s", word) != 1) return 2;
    n = word;
  }
  if (fscanf(f, "%lu %lu %lu", &nA, &first, &nRows) != 3) return 2;
  std::vector<gx_region> regions(nA);
  std::vector<gx_anchor> anchors(nA);
  std::vector<std::string> rowNames(nA);
  std::vector<const char*> rowNamePtr(nA);
  for (unsigned long a = 0; a < nA; a++) {
    int strand = 0;
    if (fscanf(f, "%u %u %u %255s %d", &regions[a].chrom, &regions[a].start, &regions[a].end, word, &strand) != 5) return 2;
    rowNames[a] = word;
    anchors[a] = gx_anchor{regions[a].chrom, regions[a].start, strand};
  }
  for (unsigned long a = 0; a < nA; a++) rowNamePtr[a] = rowNames[a] == "*" ? nullptr : rowNames[a].c_str();
  std::vector<int64_t> cells, row;
  for (unsigned long r = 0; r < nRows; r++) {
    if (!read_row(f, row, nb)) return 2;
    cells.insert(cells.end(), row.begin(), row.end());
  }
  cells.shrink_to_fit();
  fclose(f);

  std::vector<const char*> sn, cn;
  std::vector<const int64_t*> ap;
  for (unsigned long s = 0; s < nS; s++) {
    sn.push_back(sampleNames[s].c_str());
    ap.push_back(aggs[s].data());
  }
  for (auto& n : names) cn.push_back(n.c_str());
  if (int rc = gx_format_profile(stdout, (int)nS, sn.data(), ap.data(), counted, nb, F, B)) return 10 - rc;
  printf("--\n");
  if (int rc = gx_format_profile_rows(stdout, cn.data(), regions.data(), rowNamePtr.data(), anchors.data(), first, nRows, nb, B, cells.data()))
    return 10 - rc;
  // the argument checks: nothing written, GX_ERR_ORDER
  if (gx_format_profile(stdout, (int)nS, sn.data(), ap.data(), counted, 0, F, B) != GX_ERR_ORDER) return 3;
  if (gx_format_profile(stdout, (int)nS, sn.data(), ap.data(), counted, nb, F, 0) != GX_ERR_ORDER) return 3;
  if (nS && gx_format_profile(stdout, (int)nS, nullptr, ap.data(), counted, nb, F, B) != GX_ERR_ORDER) return 3;
  if (gx_format_profile_rows(stdout, cn.data(), regions.data(), rowNamePtr.data(), anchors.data(), first, nRows, nb, 0, cells.data()) != GX_ERR_ORDER)
    return 3;
  if (nRows && gx_format_profile_rows(stdout, cn.data(), regions.data(), rowNamePtr.data(), anchors.data(), first, nRows, nb, B, nullptr) != GX_ERR_ORDER)
    return 3;
  return 0;
}
