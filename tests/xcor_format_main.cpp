// Stand-alone driver of gx_format_xcor / gx_format_xcor_metrics / gx_xcor_metrics / gx_xcor_r (genrich_amd/csrc/gx_emit.cpp) for
// tests/test_xcor.py, which compiles it together with gx_emit.cpp under -fsanitize=address,undefined and compares its output
// with tests/xcor_ref.py.  No device and no library: the C ABI entries gx_emit.cpp's other writers call are defined here and
// never reached.
//
// Spec file (argv[1]): per case one line "S lo hi read_len", then per sample a line "rep is_ctrl n_pos n_plus n_minus rejected"
// and a line of the hi - lo + 1 pair counts, all decimal.  Output (stdout): every case's curve table, "--\n", its metrics
// table, "--\n".
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
    int S = 0, lo = 0, hi = 0, readLen = 0;
    if (fscanf(f, "%d %d %d %d", &S, &lo, &hi, &readLen) != 4) break;
    if (S < 1 || hi < lo) return 2;
    // (exact-size heap arrays: a read beyond them is the sanitizer's to catch)
    std::vector<int> rep((size_t)S), ctrl((size_t)S);
    std::vector<uint64_t> N((size_t)S), nP((size_t)S), nM((size_t)S), rej((size_t)S);
    std::vector<std::vector<uint64_t>> rows((size_t)S);
    std::vector<const uint64_t*> p;
    for (int i = 0; i < S; i++) {
      if (fscanf(f, "%d %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &rep[(size_t)i], &ctrl[(size_t)i], &N[(size_t)i], &nP[(size_t)i], &nM[(size_t)i],
                 &rej[(size_t)i]) != 6)
        return 2;
      rows[(size_t)i].resize((size_t)(hi - lo + 1));
      for (uint64_t& v : rows[(size_t)i])
        if (fscanf(f, "%" SCNu64, &v) != 1) return 2;
      p.push_back(rows[(size_t)i].data());
    }
    if (int rc = gx_format_xcor(stdout, S, rep.data(), ctrl.data(), N.data(), nP.data(), nM.data(), rej.data(), lo, hi, p.data())) return 10 - rc;
    printf("--\n");
    if (int rc = gx_format_xcor_metrics(stdout, S, rep.data(), ctrl.data(), N.data(), nP.data(), nM.data(), lo, hi, p.data(), readLen)) return 10 - rc;
    printf("--\n");
  }
  fclose(f);
  // the ends of the domain: the widest range with the largest genome; no tags at all; a single shift
  gx_xcor_metrics_t m;
  {
    const uint64_t N = (1ull << 37) - 1, nP = N / 3, nM = N / 5;
    std::vector<uint64_t> n11(2 * GX_XCOR_MAX_SHIFT + 1);
    for (size_t k = 0; k < n11.size(); k++) n11[k] = N / 15 + 7 * k;
    std::vector<double> r(n11.size());
    if (gx_xcor_r(N, nP, nM, -GX_XCOR_MAX_SHIFT, GX_XCOR_MAX_SHIFT, n11.data(), r.data()) != GX_OK || !(r.front() < r.back())) return 4;
    if (gx_xcor_metrics(N, nP, nM, -GX_XCOR_MAX_SHIFT, GX_XCOR_MAX_SHIFT, n11.data(), 101, &m) != GX_OK || !m.has_frag || m.frag_shift != GX_XCOR_MAX_SHIFT ||
        m.fragment_length != GX_XCOR_MAX_SHIFT + 1 || m.min_shift != -GX_XCOR_MAX_SHIFT || !m.has_phantom || m.phantom_shift != 100)
      return 4;
    const uint64_t zero[1] = {0};
    if (gx_xcor_metrics(1000, 0, 0, 7, 7, zero, 0, &m) != GX_OK || m.has_frag || m.has_phantom || !std::isnan(m.r_min) || !std::isnan(m.nsc) || !std::isnan(m.rsc))
      return 4;
    const uint64_t one[1] = {5};
    if (gx_xcor_metrics(1000, 5, 5, 7, 7, one, 8, &m) != GX_OK || !m.has_phantom || m.phantom_shift != 7 || m.has_frag /* (7 is within 10 of the phantom) */ ||
        m.min_shift != 7 || !(m.r_min == 1.0))
      return 4;
    if (gx_xcor_metrics(1000, 5, 5, 7, 7, one, 0, &m) != GX_OK || !m.has_frag || m.fragment_length != 8 || !(m.nsc == 1.0) || !std::isnan(m.rsc)) return 4;
  }
  // the argument checks: nothing written, GX_ERR_ORDER
  const uint64_t two[2] = {1, 2}, big[2] = {4, 0};
  double r2[2];
  if (gx_xcor_metrics(10, 3, 2, 0, 1, two, 0, nullptr) != GX_ERR_ORDER || gx_xcor_metrics(10, 3, 2, 0, 1, nullptr, 0, &m) != GX_ERR_ORDER) return 3;
  if (gx_xcor_metrics(10, 11, 2, 0, 1, two, 0, &m) != GX_ERR_ORDER || gx_xcor_metrics(10, 3, 11, 0, 1, two, 0, &m) != GX_ERR_ORDER) return 3;   // more tags than bases
  if (gx_xcor_metrics(10, 3, 3, 0, 1, big, 0, &m) != GX_ERR_ORDER) return 3;                                                                  // more pairs than tags
  if (gx_xcor_metrics(10, 3, 2, 1, 0, two, 0, &m) != GX_ERR_ORDER || gx_xcor_metrics(10, 3, 2, 0, 1, two, -1, &m) != GX_ERR_ORDER) return 3;
  if (gx_xcor_r(10, 3, 2, 0, 1, two, nullptr) != GX_ERR_ORDER || gx_xcor_r(10, 3, 2, -GX_XCOR_MAX_SHIFT - 1, -GX_XCOR_MAX_SHIFT, two, r2) != GX_ERR_ORDER) return 3;
  const int r0 = 0;
  const uint64_t n10 = 10, n3 = 3, n2 = 2, z = 0;
  const uint64_t* pt = two;
  const uint64_t* pb = big;
  if (gx_format_xcor(nullptr, 1, &r0, &r0, &n10, &n3, &n2, &z, 0, 1, &pt) != GX_ERR_ORDER || gx_format_xcor(stdout, 0, &r0, &r0, &n10, &n3, &n2, &z, 0, 1, &pt) != GX_ERR_ORDER ||
      gx_format_xcor(stdout, 1, &r0, &r0, &n10, &n3, &n2, &z, 0, 1, &pb) != GX_ERR_ORDER || gx_format_xcor(stdout, 1, &r0, &r0, &n10, &n3, &n2, nullptr, 0, 1, &pt) != GX_ERR_ORDER)
    return 3;
  if (gx_format_xcor_metrics(stdout, 1, &r0, &r0, &n10, &n3, &n2, 0, 1, &pb, 0) != GX_ERR_ORDER || gx_format_xcor_metrics(stdout, 1, &r0, &r0, &n10, &n3, &n2, 0, 1, &pt, -5) != GX_ERR_ORDER)
    return 3;
  return 0;
}
