// Stand-alone driver of gx_format_lengths / gx_format_lengths_metrics / gx_format_chrom_stats / gx_lengths_metrics
// (genrich_amd/csrc/gx_emit.cpp) for tests/test_lengths.py, which compiles it together with gx_emit.cpp under
// -fsanitize=address,undefined and compares its output with tests/lengths_ref.py.  No device and no library: the C ABI entries
// gx_emit.cpp's other writers call are defined here and never reached.
//
// Spec file (argv[1]): per case one line "S C cut_sites K" and a line of the K cuts, then C lines "name length" (the chromosome
// table), then per sample a line "rep is_ctrl k n_inverted w120_inverted", k lines "length n w120" and C lines "cn cw120
// cbases120", all decimal.  Output (stdout): every case's lengths table, "--\n", its metrics table, "--\n", its chromosome
// table, "--\n".
#include <cinttypes>
#include <cmath>
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
    int S = 0, C = 0, cutSites = 0, K = 0;
    if (fscanf(f, "%d %d %d %d", &S, &C, &cutSites, &K) != 4) break;
    // (exact-size heap arrays: a read beyond them is the sanitizer's to catch)
    std::vector<uint64_t> cuts((size_t)K);
    for (int k = 0; k < K; k++)
      if (fscanf(f, "%" SCNu64, &cuts[(size_t)k]) != 1) return 2;
    std::vector<std::string> names((size_t)C);
    std::vector<uint32_t> lens((size_t)C);
    for (int c = 0; c < C; c++) {
      char buf[256];
      if (fscanf(f, "%255s %" SCNu32, buf, &lens[(size_t)c]) != 2) return 2;
      names[(size_t)c] = buf;
    }
    std::vector<const char*> pn;
    for (const std::string& s : names) pn.push_back(s.c_str());
    std::vector<int> rep((size_t)S), ctrl((size_t)S);
    std::vector<uint64_t> nInv((size_t)S), wInv((size_t)S);
    std::vector<size_t> nc((size_t)S);
    std::vector<std::vector<uint64_t>> arr((size_t)S * 6);
    std::vector<const uint64_t*> p[6];
    for (int i = 0; i < S; i++) {
      size_t k = 0;
      if (fscanf(f, "%d %d %zu %" SCNu64 " %" SCNu64, &rep[(size_t)i], &ctrl[(size_t)i], &k, &nInv[(size_t)i], &wInv[(size_t)i]) != 5) return 2;
      std::vector<uint64_t>* a = &arr[(size_t)i * 6];
      for (int j = 0; j < 3; j++) a[j].resize(k);
      for (int j = 3; j < 6; j++) a[j].resize((size_t)C);
      for (size_t j = 0; j < k; j++)
        if (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64, &a[0][j], &a[1][j], &a[2][j]) != 3) return 2;
      for (int c = 0; c < C; c++)
        if (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64, &a[3][(size_t)c], &a[4][(size_t)c], &a[5][(size_t)c]) != 3) return 2;
      nc[(size_t)i] = k;
      for (int j = 0; j < 6; j++) p[j].push_back(a[j].empty() ? nullptr : a[j].data());
    }
    if (int rc = gx_format_lengths(stdout, S, rep.data(), ctrl.data(), p[0].data(), p[1].data(), p[2].data(), nc.data(), nInv.data(), wInv.data(), cutSites))
      return 10 - rc;
    printf("--\n");
    if (int rc = gx_format_lengths_metrics(stdout, S, rep.data(), ctrl.data(), p[0].data(), p[1].data(), p[2].data(), nc.data(),
                                           K ? cuts.data() : nullptr, K))
      return 10 - rc;
    printf("--\n");
    if (int rc = gx_format_chrom_stats(stdout, pn.data(), lens.data(), C, S, rep.data(), ctrl.data(), p[3].data(), p[4].data(), p[5].data())) return 10 - rc;
    printf("--\n");
  }
  fclose(f);
  // the ends of the domain: an empty sample; one class at the largest length with the largest plausible weight
  gx_len_metrics m;
  const uint64_t cuts[3] = {150, 300, 500};
  if (gx_lengths_metrics(nullptr, nullptr, nullptr, 0, cuts, 3, &m) != GX_OK || m.n != 0 || m.w120 != 0 || !std::isnan(m.mean) || !std::isnan(m.sd) ||
      m.median != 0 || m.n_shares != 4 || m.share[0] != 0.0)
    return 4;
  const uint64_t L[2] = {1, 0xFFFFFFFFull}, n[2] = {1ull << 31, 1ull << 31}, w[2] = {120ull << 31, 120ull << 31};
  if (gx_lengths_metrics(L + 1, n + 1, w + 1, 1, cuts, 3, &m) != GX_OK || std::fabs(m.mean - 4294967295.0) > 1e-3 /* (the sum has 70 bits: its leading 64 are converted) */ || m.sd != 0.0 || m.mode != L[1] || m.share[3] != 1.0) return 4;
  if (gx_lengths_metrics(L, n, w, 2, cuts, 3, &m) != GX_OK || m.mean != 2147483648.0 || std::fabs(m.sd - 2147483647.0) > 1e-3 || m.median != 1 || m.mode != 1 || m.q75 != L[1]) return 4;
  // the argument checks: nothing written, GX_ERR_ORDER
  const uint64_t down[2] = {5, 5}, zero[2] = {0, 1}, heavy[2] = {121, 121}, one[2] = {1, 1}, big[1] = {1ull << 32}, badCuts[2] = {300, 150}, nine[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
  if (gx_lengths_metrics(L, n, w, 2, cuts, 3, nullptr) != GX_ERR_ORDER || gx_lengths_metrics(nullptr, n, w, 2, cuts, 3, &m) != GX_ERR_ORDER) return 3;
  if (gx_lengths_metrics(down, n, w, 2, cuts, 3, &m) != GX_ERR_ORDER) return 3;      // lengths that do not ascend
  if (gx_lengths_metrics(L, zero, w, 2, cuts, 3, &m) != GX_ERR_ORDER) return 3;      // a class without intervals
  if (gx_lengths_metrics(L, one, heavy, 2, cuts, 3, &m) != GX_ERR_ORDER) return 3;   // more weight than intervals
  if (gx_lengths_metrics(big, one, one, 1, cuts, 3, &m) != GX_ERR_ORDER) return 3;   // a length of 2^32
  if (gx_lengths_metrics(L, n, w, 2, badCuts, 2, &m) != GX_ERR_ORDER || gx_lengths_metrics(L, n, w, 2, nine, 9, &m) != GX_ERR_ORDER ||
      gx_lengths_metrics(L, n, w, 2, zero, 2, &m) != GX_ERR_ORDER || gx_lengths_metrics(L, n, w, 2, nullptr, 1, &m) != GX_ERR_ORDER)
    return 3;
  const int r0 = 0;
  const uint64_t* pl = L;
  const uint64_t* pn2 = n;
  const uint64_t* pw = w;
  const uint64_t* pd = down;
  const size_t two = 2;
  const uint64_t z = 0;
  const char* nm = "chrA";
  const uint32_t ln = 10;
  if (gx_format_lengths(nullptr, 1, &r0, &r0, &pl, &pn2, &pw, &two, &z, &z, 0) != GX_ERR_ORDER || gx_format_lengths(stdout, 0, &r0, &r0, &pl, &pn2, &pw, &two, &z, &z, 0) != GX_ERR_ORDER ||
      gx_format_lengths(stdout, 1, &r0, &r0, &pd, &pn2, &pw, &two, &z, &z, 0) != GX_ERR_ORDER)
    return 3;
  if (gx_format_lengths_metrics(stdout, 1, &r0, &r0, &pd, &pn2, &pw, &two, cuts, 3) != GX_ERR_ORDER || gx_format_lengths_metrics(stdout, 1, &r0, &r0, &pl, &pn2, &pw, &two, badCuts, 2) != GX_ERR_ORDER)
    return 3;
  if (gx_format_chrom_stats(stdout, &nm, &ln, 0, 1, &r0, &r0, &pl, &pl, &pl) != GX_ERR_ORDER || gx_format_chrom_stats(stdout, &nm, nullptr, 1, 1, &r0, &r0, &pl, &pl, &pl) != GX_ERR_ORDER)
    return 3;
  return 0;
}
