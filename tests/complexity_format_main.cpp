// Stand-alone driver of gx_format_complexity / gx_format_complexity_hist / gx_complexity_metrics (genrich_amd/csrc/gx_emit.cpp)
// for tests/test_complexity.py, which compiles it together with gx_emit.cpp under -fsanitize=address,undefined and compares its
// output with tests/complexity_ref.py.  No device and no library: the C ABI entries gx_emit.cpp's other writers call are
// defined here and never reached.
//
// Spec file (argv[1]): per case one line "S", then per sample a line "rep is_ctrl N D m" and m lines "multiplicity keys"
// (decimal).  Output (stdout): every case's metrics table, "--\n", its histogram table, "--\n".
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
    std::vector<int> rep((size_t)S), ctrl((size_t)S);
    std::vector<uint64_t> N((size_t)S), D((size_t)S);
    std::vector<std::vector<uint64_t>> mult((size_t)S), keys((size_t)S);
    std::vector<const uint64_t*> pm((size_t)S), pk((size_t)S);
    std::vector<size_t> np((size_t)S);
    for (int i = 0; i < S; i++) {
      size_t m = 0;
      if (fscanf(f, "%d %d %" SCNu64 " %" SCNu64 " %zu", &rep[i], &ctrl[i], &N[i], &D[i], &m) != 5) return 2;
      mult[i].resize(m);
      keys[i].resize(m);
      for (size_t j = 0; j < m; j++)
        if (fscanf(f, "%" SCNu64 " %" SCNu64, &mult[i][j], &keys[i][j]) != 2) return 2;
      np[i] = m;
      pm[i] = m ? mult[i].data() : nullptr;
      pk[i] = m ? keys[i].data() : nullptr;
    }
    if (int rc = gx_format_complexity(stdout, S, rep.data(), ctrl.data(), N.data(), D.data(), pm.data(), pk.data(), np.data())) return 10 - rc;
    printf("--\n");
    if (int rc = gx_format_complexity_hist(stdout, S, rep.data(), ctrl.data(), pm.data(), pk.data(), np.data())) return 10 - rc;
    printf("--\n");
  }
  fclose(f);
  // the ends of the domain: nothing observed; one key seen 2^40 times
  gx_cpx_metrics m;
  if (gx_complexity_metrics(0, 0, nullptr, nullptr, 0, &m) != GX_OK || !std::isnan(m.nrf) || !std::isnan(m.library_size) || m.curve[19] != 0) return 4;
  const uint64_t big = (uint64_t)1 << 40, one = 1;
  if (gx_complexity_metrics(big, 1, &big, &one, 1, &m) != GX_OK || m.curve[19] != 1.0 || m.pbc1 != 0.0 || !std::isnan(m.pbc2)) return 4;
  // the argument checks: nothing written, GX_ERR_ORDER
  const int r0 = 0, c0 = 0;
  const uint64_t n3 = 3, d2 = 2, mu[2] = {1, 2}, ke[2] = {1, 1}, unsorted[2] = {2, 1}, zero[2] = {0, 3};
  const uint64_t* pmu = mu;
  const uint64_t* pke = ke;
  const size_t two = 2;
  if (gx_complexity_metrics(n3, d2, mu, ke, 2, &m) != GX_OK) return 3;
  if (gx_complexity_metrics(n3, d2, mu, ke, 2, nullptr) != GX_ERR_ORDER) return 3;
  if (gx_complexity_metrics(n3 + 1, d2, mu, ke, 2, &m) != GX_ERR_ORDER) return 3;     // sum m h[m] != N
  if (gx_complexity_metrics(n3, d2 + 1, mu, ke, 2, &m) != GX_ERR_ORDER) return 3;     // sum h[m] != D
  if (gx_complexity_metrics(n3, d2, unsorted, ke, 2, &m) != GX_ERR_ORDER) return 3;   // not ascending
  if (gx_complexity_metrics(n3, d2, zero, ke, 2, &m) != GX_ERR_ORDER) return 3;       // a multiplicity of 0
  if (gx_complexity_metrics(n3, d2, nullptr, ke, 2, &m) != GX_ERR_ORDER) return 3;
  if (gx_format_complexity(nullptr, 1, &r0, &c0, &n3, &d2, &pmu, &pke, &two) != GX_ERR_ORDER) return 3;
  if (gx_format_complexity(stdout, 0, &r0, &c0, &n3, &d2, &pmu, &pke, &two) != GX_ERR_ORDER) return 3;
  if (gx_format_complexity(stdout, 1, &r0, &c0, &n3, &d2, &pmu, nullptr, &two) != GX_ERR_ORDER) return 3;
  if (gx_format_complexity(stdout, 1, &r0, &c0, &n3, &d2, &pke, &pmu, &two) != GX_ERR_ORDER) return 3;   // (the two swapped: no histogram of N and D)
  if (gx_format_complexity_hist(nullptr, 1, &r0, &c0, &pmu, &pke, &two) != GX_ERR_ORDER) return 3;
  if (gx_format_complexity_hist(stdout, 1, &r0, &c0, &pmu, nullptr, &two) != GX_ERR_ORDER) return 3;
  return 0;
}
