// gx_emit.cpp -- host-side text emitters of the drop-in surface: ENCODE narrowPeak (-o), the
// bedgraph-ish log (-f), the pileup log (-k), the binned coverage tracks (--coverage), the profile tables (--profile), the correlation matrix (--correlation), the fingerprint tables (--fingerprint), the library complexity tables (--complexity), the interval length and chromosome tables (--lengths, --chrom-stats), the strand cross-correlation tables (--xcor), the depth distribution tables (--depth), the per-peak signal table (--peak-signal) the saturation table (--saturation) and the reproducibility tables with their support walk and figures (--reproducibility).  Pure formatting of arrays fetched through the
// C ABI (gx_get_peaks / gx_get_intervals); byte format follows the reference's printf calls:
//   printPeak       Genrich.c:885-909      printLogHeader 674-717
//   printInterval   770-803                printIntervalN 724-763
//   printPileHeader 1680-1691              printPile      1697-1715
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/genrich_amd.h"
#include "gx_fp_class.h"
#include "gx_peak_merge.h"

namespace {

struct Iv {
  std::vector<uint32_t> end;
  std::vector<float> expt, ctrl, p, q;
  size_t n = 0;
};

// --correlation's exact arithmetic: unsigned 256-bit integers, words least significant first
typedef unsigned __int128 u128_t;
struct U256 {
  uint64_t w[4] = {0, 0, 0, 0};
};
U256 mul128(u128_t a, u128_t b) {   // (schoolbook over 64-bit words; the top word cannot overflow)
  const uint64_t x[2] = {(uint64_t)a, (uint64_t)(a >> 64)}, y[2] = {(uint64_t)b, (uint64_t)(b >> 64)};
  U256 r;
  for (int i = 0; i < 2; i++) {
    uint64_t carry = 0;
    for (int j = 0; j < 2; j++) {
      const u128_t t = (u128_t)x[i] * y[j] + r.w[i + j] + carry;
      r.w[i + j] = (uint64_t)t;
      carry = (uint64_t)(t >> 64);
    }
    r.w[i + 2] = carry;
  }
  return r;
}
int cmp256(const U256& a, const U256& b) {
  for (int k = 3; k >= 0; k--)
    if (a.w[k] != b.w[k]) return a.w[k] < b.w[k] ? -1 : 1;
  return 0;
}
U256 sub256(const U256& a, const U256& b) {   // a >= b
  U256 r;
  uint64_t borrow = 0;
  for (int k = 0; k < 4; k++) {
    const u128_t t = (u128_t)a.w[k] - b.w[k] - borrow;
    r.w[k] = (uint64_t)t;
    borrow = (uint64_t)(t >> 64) & 1;
  }
  return r;
}
U256 u256_of(u128_t a) {
  U256 r;
  r.w[0] = (uint64_t)a;
  r.w[1] = (uint64_t)(a >> 64);
  return r;
}
U256 add256(const U256& a, const U256& b) {   // (no sum here reaches 2^256)
  U256 r;
  uint64_t carry = 0;
  for (int k = 0; k < 4; k++) {
    const u128_t t = (u128_t)a.w[k] + b.w[k] + carry;
    r.w[k] = (uint64_t)t;
    carry = (uint64_t)(t >> 64);
  }
  return r;
}
U256 mul256_64(const U256& a, uint64_t b) {   // (the product stays below 2^256 for every caller)
  U256 r;
  uint64_t carry = 0;
  for (int k = 0; k < 4; k++) {
    const u128_t t = (u128_t)a.w[k] * b + carry;
    r.w[k] = (uint64_t)t;
    carry = (uint64_t)(t >> 64);
  }
  return r;
}
double to_double(const U256& a) {   // the leading 64 bits, rounded once by the conversion, scaled
  int top = 3;
  while (top >= 0 && !a.w[top]) top--;
  if (top < 0) return 0.0;
  const int lz = __builtin_clzll(a.w[top]);
  uint64_t m = a.w[top] << lz;
  if (lz && top > 0) m |= a.w[top - 1] >> (64 - lz);
  return std::ldexp((double)m, 64 * top - lz);
}
// a - b as a double, the difference itself exact; *zero: it is 0
double diff256(const U256& a, const U256& b, bool* zero) {
  const int c = cmp256(a, b);
  if (zero) *zero = c == 0;
  if (c == 0) return 0.0;
  return c > 0 ? to_double(sub256(a, b)) : -to_double(sub256(b, a));
}

int fetch(gx_ctx* ctx, int which, int chrom, Iv& iv, bool piles, bool qv) {
  size_t n = 0;
  int rc = gx_interval_count(ctx, which, chrom, &n);
  if (rc) return rc;
  iv.n = n;
  iv.end.assign(n, 0);
  iv.p.assign(n, 0);
  iv.expt.assign(piles ? n : 0, 0);
  iv.ctrl.assign(piles ? n : 0, 0);
  iv.q.assign(qv ? n : 0, 0);
  if (!n) return GX_OK;
  return gx_get_intervals(ctx, which, chrom, n, iv.end.data(), piles ? iv.expt.data() : nullptr,
                          piles ? iv.ctrl.data() : nullptr, iv.p.data(), qv ? iv.q.data() : nullptr);
}

// --fingerprint
// a sample's n = sum of its counts and T = sum of its sums: 128 bits, so that histograms a caller makes up cannot wrap them
struct FpTotals {
  u128_t n = 0, T = 0;
};
FpTotals fp_totals(const uint64_t* count, const uint64_t* sum) {
  FpTotals t;
  for (int k = 0; k < GX_FP_NC; k++) {
    t.n += count[k];
    if (count[k]) t.T += sum[k];
  }
  return t;
}
std::string dec128(u128_t v) {
  char buf[40];
  int at = 40;
  do {
    buf[--at] = (char)('0' + (int)(v % 10));
    v /= 10;
  } while (v);
  return std::string(buf + at, buf + 40);
}
// one division of two integers (long double: 64 bits of each are kept)
long double ratio(u128_t a, u128_t b) { return (long double)a / (long double)b; }
void put_fraction(FILE* out, double v) {
  if (std::isnan(v)) fprintf(out, "\tnan");
  else fprintf(out, "\t%.6f", v);
}
}  // namespace

// gx_peak_merge.h's one function over contexts: their lists fetched (the only place that does), merged
int gx_peak_merge::merged_peaks(gx_ctx* const* ctxs, int n_ctx, Merged& m) {
  std::vector<std::vector<gx_peak>> own((size_t)std::max(n_ctx, 0));
  std::vector<const gx_peak*> lists;
  std::vector<size_t> n;
  for (size_t g = 0; g < own.size(); g++) {
    size_t k = 0;
    if (int rc = gx_peak_count(ctxs[g], &k)) return rc;
    own[g].resize(k);
    if (k)
      if (int rc = gx_get_peaks(ctxs[g], own[g].data(), k)) return rc;
    lists.push_back(own[g].data());
    n.push_back(k);
  }
  m = merge(lists.data(), n.data(), n.size());
  return GX_OK;
}

extern "C" {

// -o: one line per peak; peak_N numbers the peaks in output order (callPeaks' `count`): with several contexts (chromosomes
// sharded over GPUs), that of their merged peak lists.
int gx_write_narrowpeak_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, FILE* out) {
  gx_peak_merge::Merged m;
  if (int rc = gx_peak_merge::merged_peaks(ctxs, n_ctx, m)) return rc;
  return gx_format_narrowpeak(m.peaks.data(), m.size(), names, 0, out);
}

// ... the lines themselves, of a list: peak i is peak_<first_index + i>
int gx_format_narrowpeak(const gx_peak* peaks, size_t n, const char* const* names, int first_index, FILE* out) {
  if (n && (!peaks || !names || !out)) return GX_ERR_ORDER;
  for (size_t i = 0; i < n; i++) {
    const gx_peak& k = peaks[i];
    long start = (long)k.start, end = (long)k.end;
    // MIN((unsigned int)(1000.0f * signal / (end - start) + 0.5f), 1000): the float -> unsigned
    // conversion of an out-of-range value follows x86-64 gcc (64-bit cvttss2si, low 32 bits)
    float sc = 1000.0f * k.auc / (float)(end - start) + 0.5f;
    unsigned int u = (unsigned int)(long long)sc;
    fprintf(out, "%s\t%ld\t%ld\tpeak_%d\t%d\t.\t%f\t%f", names[k.chrom], start, end, first_index + (int)i, u < 1000u ? u : 1000u, k.auc,
            k.p);
    if (k.q == GX_SKIP)
      fprintf(out, "\t-1\t%d\n", k.summit);
    else
      fprintf(out, "\t%f\t%d\n", k.q, k.summit);
  }
  return GX_OK;
}

int gx_write_narrowpeak(gx_ctx* ctx, const char* const* names, FILE* out) { return gx_write_narrowpeak_group(&ctx, 1, names, out); }

// --counts (no Genrich counterpart): the rows of -o -- the merged peaks, the same peak_N -- with one column per sample, n / 120 of
// its count (gx_count_in_peaks on every context first)
static void put_count(FILE* out, long long n) {
  if (n % 120 == 0) fprintf(out, "\t%lld", n / 120);
  else fprintf(out, "\t%.2f", (double)n / 120.0);
}
int gx_write_counts_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, int n_samples,
                          const char* const* sample_names, FILE* out) {
  if (n_ctx < 1 || n_samples < 0 || (n_samples && !sample_names)) return GX_ERR_ORDER;
  gx_peak_merge::Merged m;
  if (int rc = gx_peak_merge::merged_peaks(ctxs, n_ctx, m)) return rc;
  std::vector<std::vector<int64_t>> cnt((size_t)n_samples);   // [sample][peak]
  for (int smp = 0; smp < n_samples; smp++) {
    cnt[smp].resize(m.size());
    for (int g = 0; g < n_ctx; g++)
      if (int rc = gx_get_peak_counts(ctxs[g], smp, nullptr, nullptr, cnt[smp].data() + m.first[g], m.first[g + 1] - m.first[g], nullptr, nullptr)) return rc;
    cnt[smp] = permuted(m, cnt[smp]);
  }
  fprintf(out, "chr\tstart\tend\tname");
  for (int smp = 0; smp < n_samples; smp++) fprintf(out, "\t%s", sample_names[smp]);
  fprintf(out, "\n");
  for (size_t i = 0; i < m.size(); i++) {
    const gx_region& k = m.regions[i];
    fprintf(out, "%s\t%ld\t%ld\tpeak_%d", names[k.chrom], (long)k.start, (long)k.end, (int)i);
    for (int smp = 0; smp < n_samples; smp++) put_count(out, (long long)cnt[smp][i]);
    fprintf(out, "\n");
  }
  return GX_OK;
}

int gx_write_counts(gx_ctx* ctx, const char* const* names, int n_samples, const char* const* sample_names, FILE* out) {
  return gx_write_counts_group(&ctx, 1, names, n_samples, sample_names, out);
}

// --peak-signal (no Genrich counterpart): the rows of --counts -- chr, start, end, peak_N in the order given -- with five
// columns per sample; host only, no context.  The figures in 1/120 units are printed as --counts prints a count.
int gx_format_peak_signal(FILE* out, const char* const* names, const gx_region* peaks, size_t n_peaks, int n_samples, const int* rep,
                          const int* is_ctrl, const int64_t* const* area120, const int64_t* const* max120, const uint32_t* const* summit,
                          const uint32_t* const* covered, const int64_t* const* at_summit120) {
  if (!out || n_samples < 0 || (n_peaks && (!peaks || !names))) return GX_ERR_ORDER;
  if (n_samples && (!rep || !is_ctrl || !area120 || !max120 || !summit || !covered || !at_summit120)) return GX_ERR_ORDER;
  for (int s = 0; n_peaks && s < n_samples; s++)
    if (!area120[s] || !max120[s] || !summit[s] || !covered[s] || !at_summit120[s]) return GX_ERR_ORDER;
  fprintf(out, "chr\tstart\tend\tname");
  for (int s = 0; s < n_samples; s++)
    for (const char* col : {"max", "summit", "area", "covered", "at_summit"}) fprintf(out, "\t%c%d.%s", is_ctrl[s] ? 'c' : 't', rep[s], col);
  fprintf(out, "\n");
  for (size_t i = 0; i < n_peaks; i++) {
    const gx_region& k = peaks[i];
    fprintf(out, "%s\t%ld\t%ld\tpeak_%d", names[k.chrom], (long)k.start, (long)k.end, (int)i);
    for (int s = 0; s < n_samples; s++) {
      put_count(out, (long long)max120[s][i]);
      fprintf(out, "\t%u", summit[s][i]);
      put_count(out, (long long)area120[s][i]);
      fprintf(out, "\t%u", covered[s][i]);
      put_count(out, (long long)at_summit120[s][i]);
    }
    fprintf(out, "\n");
  }
  return GX_OK;
}

// --summits (no Genrich counterpart): one row per summit of the pooled treatment depth, BED in its first six columns; host only,
// no context.  The summits come ascending in (peak, pos), each peak's numbered from 1; the peaks' names are the narrowPeak's.
int gx_format_summits(FILE* out, const char* const* names, const gx_region* peaks, size_t n_peaks, const gx_summit* summits, size_t n) {
  if (!out || (n && (!summits || !peaks || !names))) return GX_ERR_ORDER;
  for (size_t i = 0; i < n; i++) {
    const gx_summit& s = summits[i];
    if (s.peak >= n_peaks || s.width == 0 || s.pos < (s.width - 1) / 2) return GX_ERR_ORDER;
    const uint64_t a = s.pos - (s.width - 1) / 2;
    if (a + s.width > (uint64_t)peaks[s.peak].end - peaks[s.peak].start) return GX_ERR_ORDER;
    if (i && (summits[i - 1].peak > s.peak || (summits[i - 1].peak == s.peak && summits[i - 1].pos >= s.pos))) return GX_ERR_ORDER;
  }
  fprintf(out, "chr\tstart\tend\tname\theight\tstrand\tplateau_start\tplateau_end\tprominence\tpeak_start\tpeak_end\n");
  size_t j = 0;
  for (size_t i = 0; i < n; i++) {
    const gx_summit& s = summits[i];
    const gx_region& k = peaks[s.peak];
    j = i && summits[i - 1].peak == s.peak ? j + 1 : 1;
    const long at = (long)k.start + (long)s.pos, a = at - (long)((s.width - 1) / 2);
    fprintf(out, "%s\t%ld\t%ld\tpeak_%u.%zu", names[k.chrom], at, at + 1, s.peak, j);
    put_count(out, (long long)s.height120);
    fprintf(out, "\t.\t%ld\t%ld", a, a + (long)s.width);
    put_count(out, (long long)s.prominence120);
    fprintf(out, "\t%ld\t%ld\n", (long)k.start, (long)k.end);
  }
  return GX_OK;
}

// --region-counts: one row per region in the caller's order, the contexts' counts added (a region lies on one chromosome, which
// one context owns; the others count 0 there)
int gx_write_region_counts_group(gx_ctx* const* ctxs, int n_ctx, const char* const* names, const gx_region* regions,
                                 const char* const* region_names, size_t n, int n_samples, const char* const* sample_names,
                                 FILE* out) {
  if (n_ctx < 1 || n_samples < 0 || (n_samples && !sample_names) || (n && !regions)) return GX_ERR_ORDER;
  std::vector<int64_t> cnt(n * (size_t)n_samples, 0), one(n);   // [sample][region]
  for (int g = 0; g < n_ctx; g++)
    for (int smp = 0; smp < n_samples; smp++) {
      if (int rc = gx_get_region_counts(ctxs[g], smp, nullptr, nullptr, one.data(), n, nullptr, nullptr)) return rc;
      for (size_t i = 0; i < n; i++) cnt[(size_t)smp * n + i] += one[i];
    }
  fprintf(out, "chr\tstart\tend\tname");
  for (int smp = 0; smp < n_samples; smp++) fprintf(out, "\t%s", sample_names[smp]);
  fprintf(out, "\n");
  for (size_t i = 0; i < n; i++) {
    const gx_region& r = regions[i];
    fprintf(out, "%s\t%u\t%u\t", names[r.chrom], r.start, r.end);
    if (region_names && region_names[i]) fprintf(out, "%s", region_names[i]);
    else fprintf(out, "region_%zu", i);
    for (int smp = 0; smp < n_samples; smp++) put_count(out, (long long)cnt[(size_t)smp * n + i]);
    fprintf(out, "\n");
  }
  return GX_OK;
}

int gx_write_region_counts(gx_ctx* ctx, const char* const* names, const gx_region* regions, const char* const* region_names,
                           size_t n, int n_samples, const char* const* sample_names, FILE* out) {
  return gx_write_region_counts_group(&ctx, 1, names, regions, region_names, n, n_samples, sample_names, out);
}

// -k for replicate `rep` (owner[c] = index into ctxs of the context that computed chromosome c; NULL: ctxs[0])
int gx_write_pile_group(gx_ctx* const* ctxs, const int* owner, int rep, const char* const* names, int n_chrom,
                        const char* expt_name, const char* ctrl_name, FILE* out) {
  fprintf(out, "# experimental file: %s; control file: %s\n", expt_name,
          ctrl_name && strcmp(ctrl_name, "null") ? ctrl_name : "NA");
  fprintf(out, "chr\tstart\tend\texperimental\tcontrol\t-log(p)\n");
  Iv iv;
  for (int c = 0; c < n_chrom; c++) {
    int rc = fetch(ctxs[owner ? owner[c] : 0], rep, c, iv, true, false);
    if (rc) return rc;
    uint32_t start = 0;
    for (size_t m = 0; m < iv.n; m++) {
      if (iv.ctrl[m] == GX_SKIP)
        fprintf(out, "%s\t%d\t%d\t%f\t%f\t%s\n", names[c], start, iv.end[m], iv.expt[m], 0.0f, "NA");
      else
        fprintf(out, "%s\t%d\t%d\t%f\t%f\t%f\n", names[c], start, iv.end[m], iv.expt[m], iv.ctrl[m], iv.p[m]);
      start = iv.end[m];
    }
  }
  return GX_OK;
}

int gx_write_pile(gx_ctx* ctx, int rep, const char* const* names, int n_chrom, const char* expt_name,
                  const char* ctrl_name, FILE* out) {
  return gx_write_pile_group(&ctx, nullptr, rep, names, n_chrom, expt_name, ctrl_name, out);
}

// --coverage: bedGraph lines of one chromosome's bins.  Adjacent bins with exactly equal means (cross-multiplied in 128 bits:
// the chromosome's last bin may be short) share a line; a line's value is its sum over its bases.
int gx_format_coverage(FILE* out, const char* chrom_name, uint32_t len, uint32_t bin_size, const int64_t* sum120, size_t n_bins,
                       double scale) {
  if (!out || !chrom_name || !bin_size || (n_bins && !sum120)) return GX_ERR_ORDER;
  if (n_bins != ((size_t)len + bin_size - 1) / bin_size) return GX_ERR_ORDER;
  size_t a = 0;
  while (a < n_bins) {
    const uint64_t start = (uint64_t)a * bin_size;
    const uint64_t firstBases = std::min<uint64_t>(start + bin_size, len) - start;
    __int128 sum = sum120[a];
    uint64_t bases = firstBases;
    size_t b = a + 1;
    for (; b < n_bins; b++) {
      const uint64_t s0 = (uint64_t)b * bin_size, nb = std::min<uint64_t>(s0 + bin_size, len) - s0;
      if ((__int128)sum120[a] * (__int128)nb != (__int128)sum120[b] * (__int128)firstBases) break;
      sum += sum120[b];
      bases += nb;
    }
    const __int128 unit = (__int128)120 * (__int128)bases;
    if (scale == 1.0 && sum % unit == 0)
      fprintf(out, "%s\t%llu\t%llu\t%lld\n", chrom_name, (unsigned long long)start, (unsigned long long)(start + bases),
              (long long)(sum / unit));
    else
      fprintf(out, "%s\t%llu\t%llu\t%.4f\n", chrom_name, (unsigned long long)start, (unsigned long long)(start + bases),
              ((double)sum / (120.0 * (double)bases)) * scale);
    a = b;
  }
  return GX_OK;
}

int gx_write_coverage_group(gx_ctx* const* ctxs, const int* owner, int sample, const char* const* names, int n_chrom, double scale,
                            FILE* out) {
  if (!ctxs || !names || !out) return GX_ERR_ORDER;
  std::vector<int64_t> sums;
  for (int c = 0; c < n_chrom; c++) {
    gx_ctx* ctx = ctxs[owner ? owner[c] : 0];
    size_t n = 0;
    uint32_t W = 0, len = 0;
    int rc = gx_coverage_bin_count(ctx, c, &n);
    if (!rc) rc = gx_coverage_layout(ctx, c, &W, &len);
    if (rc) return rc;
    if (!n) continue;
    sums.assign(n, 0);
    if ((rc = gx_get_coverage(ctx, sample, c, nullptr, nullptr, sums.data(), n))) return rc;
    if ((rc = gx_format_coverage(out, names[c], len, W, sums.data(), n, scale))) return rc;
  }
  return GX_OK;
}

int gx_write_coverage(gx_ctx* ctx, int sample, const char* const* names, int n_chrom, double scale, FILE* out) {
  return gx_write_coverage_group(&ctx, nullptr, sample, names, n_chrom, scale, out);
}

// --profile: the aggregate table, one column per sample
int gx_format_profile(FILE* out, int n_samples, const char* const* sample_names, const int64_t* const* agg120, size_t n_anchors_counted,
                      uint32_t n_bins, uint32_t flank, uint32_t bin_size) {
  if (!out || n_samples < 0 || (n_samples && (!sample_names || !agg120)) || !n_bins || !bin_size) return GX_ERR_ORDER;
  for (int smp = 0; smp < n_samples; smp++)
    if (!sample_names[smp] || !agg120[smp]) return GX_ERR_ORDER;
  fprintf(out, "offset");
  for (int smp = 0; smp < n_samples; smp++) fprintf(out, "\t%s", sample_names[smp]);
  fprintf(out, "\n");
  for (uint32_t j = 0; j < n_bins; j++) {
    fprintf(out, "%lld", (long long)j * (long long)bin_size - (long long)flank);
    for (int smp = 0; smp < n_samples; smp++)
      fprintf(out, "\t%.6f", n_anchors_counted ? (double)agg120[smp][j] / (120.0 * bin_size * n_anchors_counted) : 0.0);
    fprintf(out, "\n");
  }
  return GX_OK;
}

// ... and rows of a sample's matrix, one per anchor (--coverage's value rule over bin_size bases)
int gx_format_profile_rows(FILE* out, const char* const* names, const gx_region* regions, const char* const* row_names,
                           const gx_anchor* anchors, size_t first, size_t n_rows, uint32_t n_bins, uint32_t bin_size,
                           const int64_t* cell120) {
  if (!out || !n_bins || !bin_size || (n_rows && (!names || !regions || !anchors || !cell120))) return GX_ERR_ORDER;
  const long long unit = 120ll * (long long)bin_size;
  for (size_t i = 0; i < n_rows; i++) {
    const size_t a = first + i;
    const gx_region& r = regions[a];
    fprintf(out, "%s\t%u\t%u\t", names[r.chrom], r.start, r.end);
    if (row_names && row_names[a]) fprintf(out, "%s", row_names[a]);
    else fprintf(out, "anchor_%zu", a);
    fprintf(out, "\t%c", anchors[a].strand < 0 ? '-' : '+');
    const int64_t* row = cell120 + i * (size_t)n_bins;
    for (uint32_t j = 0; j < n_bins; j++) {
      if (row[j] % unit == 0) fprintf(out, "\t%lld", (long long)(row[j] / unit));
      else fprintf(out, "\t%.4f", (double)row[j] / (120.0 * (double)bin_size));
    }
    fprintf(out, "\n");
  }
  return GX_OK;
}

// --correlation: the Pearson matrix from the exact sums; NaN where there is no correlation
int gx_correlation_matrix(int n_samples, uint64_t n, uint64_t n_zero, const gx_u128* sum, const gx_u128* gram, int skip_zeros, double* r) {
  if (n_samples < 1 || !sum || !gram || !r || n_zero > n) return GX_ERR_ORDER;
  const size_t S = (size_t)n_samples;
  const uint64_t N = skip_zeros ? n - n_zero : n;
  auto v = [](const gx_u128& x) { return ((u128_t)x.hi << 64) | x.lo; };
  std::vector<double> var(S);
  std::vector<char> flat(S);
  for (size_t i = 0; i < S; i++) {
    bool zero = false;
    var[i] = diff256(mul128(N, v(gram[i * S + i])), mul128(v(sum[i]), v(sum[i])), &zero);
    flat[i] = zero || N < 2;
  }
  for (size_t i = 0; i < S; i++)
    for (size_t j = 0; j < S; j++) {
      if (i == j) r[i * S + j] = 1.0;
      else if (flat[i] || flat[j]) r[i * S + j] = std::nan("");
      else r[i * S + j] = diff256(mul128(N, v(gram[i * S + j])), mul128(v(sum[i]), v(sum[j])), nullptr) / std::sqrt(var[i] * var[j]);
    }
  return GX_OK;
}

// ... and its text
int gx_format_correlation(FILE* out, int n_samples, const char* const* sample_names, uint64_t n, uint64_t n_zero, const gx_u128* sum,
                          const gx_u128* gram, int skip_zeros) {
  if (!out || n_samples < 1 || !sample_names) return GX_ERR_ORDER;
  const size_t S = (size_t)n_samples;
  for (size_t i = 0; i < S; i++)
    if (!sample_names[i]) return GX_ERR_ORDER;
  std::vector<double> r(S * S);
  if (int rc = gx_correlation_matrix(n_samples, n, n_zero, sum, gram, skip_zeros, r.data())) return rc;
  for (size_t j = 0; j < S; j++) fprintf(out, "\t%s", sample_names[j]);
  fprintf(out, "\n");
  for (size_t i = 0; i < S; i++) {
    fprintf(out, "%s", sample_names[i]);
    for (size_t j = 0; j < S; j++) {
      if (i == j) fprintf(out, "\t1.000000");
      else if (std::isnan(r[i * S + j])) fprintf(out, "\tnan");
      else fprintf(out, "\t%.6f", r[i * S + j]);
    }
    fprintf(out, "\n");
  }
  return GX_OK;
}

// --spearman: the contexts' (value, count) tables of every sample merged into one table (value, rank2) per sample
int gx_rank_tables(int n_ctx, int n_samples, const gx_rank_table* tables, uint64_t n_zero_to_drop, uint64_t* const* value,
                   uint64_t* const* rank2, size_t cap, size_t* n_out, uint64_t* n_ranked) {
  if (n_ctx < 1 || n_samples < 1 || n_samples > 32 || !tables || !n_out || ((value == nullptr) != (rank2 == nullptr))) return GX_ERR_ORDER;
  const size_t S = (size_t)n_samples, G = (size_t)n_ctx;
  uint64_t N = 0;
  std::vector<std::pair<uint64_t, uint64_t>> all, merged;
  for (size_t s = 0; s < S; s++) {
    all.clear();
    merged.clear();
    for (size_t g = 0; g < G; g++) {
      const gx_rank_table& t = tables[g * S + s];
      if (t.n && (!t.value || !t.count)) return GX_ERR_ORDER;
      for (size_t k = 0; k < t.n; k++) {
        if ((k && t.value[k - 1] >= t.value[k]) || !t.count[k] || t.count[k] >> 41) return GX_ERR_ORDER;
        all.emplace_back(t.value[k], t.count[k]);
      }
    }
    std::sort(all.begin(), all.end());
    for (const auto& p : all) {
      if (!merged.empty() && merged.back().first == p.first) merged.back().second += p.second;
      else merged.push_back(p);
      if (merged.back().second >> 41) return GX_ERR_ORDER;
    }
    if (n_zero_to_drop) {   // (the bins that are 0 in every sample are 0 in this one)
      if (merged.empty() || merged[0].first != 0 || merged[0].second < n_zero_to_drop) return GX_ERR_ORDER;
      merged[0].second -= n_zero_to_drop;
      if (!merged[0].second) merged.erase(merged.begin());
    }
    uint64_t total = 0;
    for (const auto& p : merged) {
      total += p.second;
      if (total >> 41) return GX_ERR_ORDER;   // N < 2^41: a rank below 2^42, a sum of products below 2^125
    }
    if (s == 0) N = total;
    else if (total != N) return GX_ERR_ORDER;   // (every sample has the same bins)
    n_out[s] = merged.size();
    if (!value) continue;
    if (merged.size() > cap || (!merged.empty() && (!value[s] || !rank2[s]))) return GX_ERR_ORDER;
    uint64_t less = 0;
    for (size_t k = 0; k < merged.size(); k++) {
      value[s][k] = merged[k].first;
      rank2[s][k] = 2 * less + merged[k].second + 1;
      less += merged[k].second;
    }
  }
  if (n_ranked) *n_ranked = N;
  return GX_OK;
}

// --fingerprint: the value classes (gx_fp_class.h) behind the C ABI
uint32_t gx_fp_class(uint64_t x) { return gx::fp_class(x); }
uint64_t gx_fp_class_lo(uint32_t k) { return k < (uint32_t)GX_FP_NC ? gx::fp_class_lo(k) : 0; }
uint64_t gx_fp_class_hi(uint32_t k) { return k < (uint32_t)GX_FP_NC ? gx::fp_class_hi(k) : 0; }

// --fingerprint's figures, from the integers alone: NaN where a definition divides by 0
int gx_fingerprint_metrics(int n_samples, const uint64_t* count, const uint64_t* sum, const int* ctrl_of, gx_fp_metrics* out) {
  if (n_samples < 1 || !count || !sum || !out) return GX_ERR_ORDER;
  const double nan = std::nan("");
  for (int s = 0; s < n_samples; s++) {
    if (ctrl_of && (ctrl_of[s] >= n_samples || ctrl_of[s] == s)) return GX_ERR_ORDER;
    const uint64_t* c = count + (size_t)s * GX_FP_NC;
    const uint64_t* v = sum + (size_t)s * GX_FP_NC;
    const FpTotals t = fp_totals(c, v);
    gx_fp_metrics m{nan, nan, nan, nan, nan, nan};
    if (t.n) m.zero_fraction = (double)ratio(c[0], t.n);
    if (t.n && t.T) {
      long double auc = 0, p0 = 0, l0 = 0, best = -1;
      u128_t C = 0, L = 0;
      for (int k = 0; k < GX_FP_NC; k++) {
        if (!c[k]) continue;
        C += c[k];
        L += v[k];
        const long double p = ratio(C, t.n), l = ratio(L, t.T);
        auc += (p - p0) * (l + l0) / 2;
        if (p - l > best) {
          best = p - l;
          m.elbow_bins = (double)p;
          m.elbow_gap = (double)(p - l);
        }
        p0 = p;
        l0 = l;
      }
      m.auc = (double)auc;
      m.gini = (double)(1 - 2 * auc);
    }
    const int ct = ctrl_of ? ctrl_of[s] : -1;
    if (ct >= 0 && t.n) {
      const uint64_t* cc = count + (size_t)ct * GX_FP_NC;
      const FpTotals tc = fp_totals(cc, sum + (size_t)ct * GX_FP_NC);
      if (tc.n) {
        long double js = 0;
        for (int k = 0; k < GX_FP_NC; k++) {
          if (!c[k] && !cc[k]) continue;
          const long double p = ratio(c[k], t.n), q = ratio(cc[k], tc.n), mid = (p + q) / 2;
          if (c[k]) js += p * std::log2(p / mid) / 2;
          if (cc[k]) js += q * std::log2(q / mid) / 2;
        }
        m.jsd_control = (double)std::sqrt(std::max<long double>(js, 0));
      }
    }
    out[s] = m;
  }
  return GX_OK;
}

// ... the curve table: one row per sample and non-empty class
int gx_format_fingerprint(FILE* out, int n_samples, const char* const* sample_names, const uint64_t* count, const uint64_t* sum) {
  if (!out || n_samples < 1 || !sample_names || !count || !sum) return GX_ERR_ORDER;
  for (int s = 0; s < n_samples; s++)
    if (!sample_names[s]) return GX_ERR_ORDER;
  fprintf(out, "sample\tlo120\thi120\tbins\tsum120\tcum_bins\tcum_signal\n");
  for (int s = 0; s < n_samples; s++) {
    const uint64_t* c = count + (size_t)s * GX_FP_NC;
    const uint64_t* v = sum + (size_t)s * GX_FP_NC;
    const FpTotals t = fp_totals(c, v);
    u128_t C = 0, L = 0;
    for (int k = 0; k < GX_FP_NC; k++) {
      if (!c[k]) continue;
      C += c[k];
      L += v[k];
      fprintf(out, "%s\t%llu\t%llu\t%llu\t%llu", sample_names[s], (unsigned long long)gx::fp_class_lo((uint32_t)k),
              (unsigned long long)gx::fp_class_hi((uint32_t)k), (unsigned long long)c[k], (unsigned long long)v[k]);
      put_fraction(out, (double)ratio(C, t.n));
      put_fraction(out, t.T ? (double)ratio(L, t.T) : std::nan(""));
      fprintf(out, "\n");
    }
  }
  return GX_OK;
}

// ... and the figures, one row per sample
int gx_format_fingerprint_metrics(FILE* out, int n_samples, const char* const* sample_names, const uint64_t* count, const uint64_t* sum,
                                  const int* ctrl_of) {
  if (!out || n_samples < 1 || !sample_names || !count || !sum) return GX_ERR_ORDER;
  for (int s = 0; s < n_samples; s++)
    if (!sample_names[s]) return GX_ERR_ORDER;
  std::vector<gx_fp_metrics> m((size_t)n_samples);
  if (int rc = gx_fingerprint_metrics(n_samples, count, sum, ctrl_of, m.data())) return rc;
  fprintf(out, "sample\tbins\tzero_bins\tsum120\tzero_fraction\tauc\tgini\telbow_bins\telbow_gap\tjsd_control\n");
  for (int s = 0; s < n_samples; s++) {
    const FpTotals t = fp_totals(count + (size_t)s * GX_FP_NC, sum + (size_t)s * GX_FP_NC);
    fprintf(out, "%s\t%s\t%llu\t%s", sample_names[s], dec128(t.n).c_str(), (unsigned long long)count[(size_t)s * GX_FP_NC], dec128(t.T).c_str());
    for (double v : {m[s].zero_fraction, m[s].auc, m[s].gini, m[s].elbow_bins, m[s].elbow_gap, m[s].jsd_control}) put_fraction(out, v);
    fprintf(out, "\n");
  }
  return GX_OK;
}

// --complexity's figures, from the integers alone: NaN where a definition divides by 0 or has no root
namespace {
// a / b, the correctly rounded double when both are below 2^53 (every count a device pass gives is); else through long double
double cpx_ratio(uint64_t a, uint64_t b) {
  if (!((a | b) >> 53)) return (double)a / (double)b;
  return (double)((long double)a / (long double)b);
}
// the X with D / X = 1 - exp(-N / X) (Lander-Waterman), 0 < D < N: g(X) = -X expm1(-N / X) - D rises from g(D) < 0 to N - D
long double cpx_library_size(uint64_t N, uint64_t D) {
  const long double n = (long double)N, d = (long double)D;
  auto g = [&](long double X) { return -X * expm1l(-n / X) - d; };
  long double lo = d, hi = d;
  do hi *= 2;
  while (g(hi) < 0 && hi < 0x1p1000L);
  for (int it = 0; it < 400; it++) {
    const long double mid = lo + (hi - lo) / 2;
    if (mid <= lo || mid >= hi) break;
    if (g(mid) < 0) lo = mid;
    else hi = mid;
  }
  return lo + (hi - lo) / 2;
}
bool cpx_pairs_ok(uint64_t N, uint64_t D, const uint64_t* mult, const uint64_t* keys, size_t n_pairs) {
  if (n_pairs && (!mult || !keys)) return false;
  u128_t sh = 0, smh = 0;
  for (size_t i = 0; i < n_pairs; i++) {
    if (!mult[i] || !keys[i] || (i && mult[i - 1] >= mult[i])) return false;
    sh += keys[i];
    smh += (u128_t)mult[i] * keys[i];
    if (smh > N) return false;
  }
  return sh == D && smh == N;
}
void put_cpx(FILE* out, double v, const char* fmt) {
  if (std::isnan(v)) fprintf(out, "\tNA");
  else fprintf(out, fmt, v);
}
}  // namespace

int gx_complexity_metrics(uint64_t n_obs, uint64_t n_distinct, const uint64_t* mult, const uint64_t* keys, size_t n_pairs, gx_cpx_metrics* out) {
  if (!out || !cpx_pairs_ok(n_obs, n_distinct, mult, keys, n_pairs)) return GX_ERR_ORDER;
  const uint64_t N = n_obs, D = n_distinct;
  const double nan = std::nan("");
  gx_cpx_metrics m{};
  for (size_t i = 0; i < n_pairs; i++) {
    if (mult[i] == 1) m.h1 = keys[i];
    if (mult[i] == 2) m.h2 = keys[i];
  }
  m.nrf = N ? cpx_ratio(D, N) : nan;
  m.pbc1 = D ? cpx_ratio(m.h1, D) : nan;
  m.pbc2 = m.h2 ? cpx_ratio(m.h1, m.h2) : nan;
  m.dup_fraction = N ? cpx_ratio(N - D, N) : nan;
  m.library_size = (N && D < N) ? (double)roundl(cpx_library_size(N, D)) : nan;
  for (int k = 1; k <= GX_CPX_CURVE; k++) {
    const uint64_t n = (uint64_t)(((u128_t)N * (unsigned)k + GX_CPX_CURVE / 2) / GX_CPX_CURVE);   // round(k N / 20), halves up
    long double E = 0;
    for (size_t i = 0; i < n_pairs; i++) {
      // the chance that none of a key's m observations is among the n drawn: prod_{i < m} (N - n - i) / (N - i), factor by
      // factor until it is 0 (m > N - n) or too small to show in 1 - p (below 2^-80)
      long double p = 1;
      for (uint64_t j = 0; j < mult[i] && p >= 0x1p-80L; j++) p = j >= N - n ? 0.0L : p * ((long double)(N - n - j) / (long double)(N - j));
      if (p < 0x1p-80L) p = 0;
      E += (long double)keys[i] * (1 - p);
    }
    m.curve[k - 1] = (double)E;
  }
  *out = m;
  return GX_OK;
}

// ... one row per sample, labelled t<rep> / c<rep>
int gx_format_complexity(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* n_obs, const uint64_t* n_distinct,
                         const uint64_t* const* mult, const uint64_t* const* keys, const size_t* n_pairs) {
  if (!out || n_samples < 1 || !rep || !is_ctrl || !n_obs || !n_distinct || !mult || !keys || !n_pairs) return GX_ERR_ORDER;
  std::vector<gx_cpx_metrics> m((size_t)n_samples);
  for (int s = 0; s < n_samples; s++)
    if (int rc = gx_complexity_metrics(n_obs[s], n_distinct[s], mult[s], keys[s], n_pairs[s], &m[s])) return rc;
  fprintf(out, "sample\tN\tD\th1\th2\tNRF\tPBC1\tPBC2\tdup_fraction\tlibrary_size");
  for (int k = 1; k <= GX_CPX_CURVE; k++) fprintf(out, "\tc%03d", k * 100 / GX_CPX_CURVE);
  fprintf(out, "\n");
  for (int s = 0; s < n_samples; s++) {
    fprintf(out, "%c%d\t%llu\t%llu\t%llu\t%llu", is_ctrl[s] ? 'c' : 't', rep[s], (unsigned long long)n_obs[s], (unsigned long long)n_distinct[s],
            (unsigned long long)m[s].h1, (unsigned long long)m[s].h2);
    for (double v : {m[s].nrf, m[s].pbc1, m[s].pbc2, m[s].dup_fraction}) put_cpx(out, v, "\t%.6f");
    put_cpx(out, m[s].library_size, "\t%.0f");
    for (int k = 0; k < GX_CPX_CURVE; k++) put_cpx(out, m[s].curve[k], "\t%.3f");
    fprintf(out, "\n");
  }
  return GX_OK;
}

// ... and the sparse histogram: sample, multiplicity, keys
int gx_format_complexity_hist(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* const* mult,
                              const uint64_t* const* keys, const size_t* n_pairs) {
  if (!out || n_samples < 1 || !rep || !is_ctrl || !mult || !keys || !n_pairs) return GX_ERR_ORDER;
  for (int s = 0; s < n_samples; s++)
    if (n_pairs[s] && (!mult[s] || !keys[s])) return GX_ERR_ORDER;
  fprintf(out, "sample\tmultiplicity\tkeys\n");
  for (int s = 0; s < n_samples; s++)
    for (size_t i = 0; i < n_pairs[s]; i++)
      fprintf(out, "%c%d\t%llu\t%llu\n", is_ctrl[s] ? 'c' : 't', rep[s], (unsigned long long)mult[s][i], (unsigned long long)keys[s][i]);
  return GX_OK;
}

// --lengths / --lengths-metrics / --chrom-stats: the figures from the integers alone
namespace {
// a sample's lengths as the device pass gives them: strictly ascending and below 2^32, every class with intervals whose weight
// lies between 1/120 and 1 each; *W: the weight of all of them
bool len_classes_ok(const uint64_t* length, const uint64_t* n, const uint64_t* w120, size_t n_classes, uint64_t* N, uint64_t* W) {
  if (n_classes && (!length || !n || !w120)) return false;
  u128_t sn = 0, sw = 0;
  for (size_t i = 0; i < n_classes; i++) {
    if ((length[i] >> 32) || (i && length[i - 1] >= length[i]) || !n[i] || w120[i] < n[i] || (u128_t)w120[i] > (u128_t)120 * n[i]) return false;
    sn += n[i];
    sw += w120[i];
  }
  if ((sn >> 64) || (sw >> 64)) return false;
  *N = (uint64_t)sn;
  *W = (uint64_t)sw;
  return true;
}
bool len_cuts_ok(const uint64_t* cuts, int n_cuts) {
  if (n_cuts < 0 || n_cuts > GX_LEN_MAX_CUTS || (n_cuts && !cuts)) return false;
  for (int k = 0; k < n_cuts; k++)
    if (!cuts[k] || (k && cuts[k - 1] >= cuts[k])) return false;
  return true;
}
void put_w120(FILE* out, uint64_t w) {   // a weight in 1/120 units, as --counts prints one
  if (w % 120 == 0) fprintf(out, "\t%llu", (unsigned long long)(w / 120));
  else fprintf(out, "\t%.2f", (double)w / 120.0);
}
}  // namespace

int gx_lengths_metrics(const uint64_t* length, const uint64_t* n, const uint64_t* w120, size_t n_classes, const uint64_t* cuts, int n_cuts,
                       gx_len_metrics* out) {
  uint64_t N = 0, W = 0;
  if (!out || !len_cuts_ok(cuts, n_cuts) || !len_classes_ok(length, n, w120, n_classes, &N, &W)) return GX_ERR_ORDER;
  gx_len_metrics m{};
  const double nan = std::nan("");
  m.n = N;
  m.w120 = W;
  m.n_shares = n_cuts + 1;
  m.mean = m.sd = nan;
  if (!n_classes) {
    *out = m;
    return GX_OK;
  }
  m.min = length[0];
  m.max = length[n_classes - 1];
  // sum w L (below 2^128: w < 2^64, L < 2^32, fewer than 2^32 classes) and sum w L^2, exact
  u128_t swl = 0;
  U256 swl2;
  uint64_t best = 0;
  for (size_t i = 0; i < n_classes; i++) {
    swl += (u128_t)w120[i] * length[i];
    swl2 = add256(swl2, mul128((u128_t)w120[i], (u128_t)length[i] * length[i]));
    if (w120[i] > best) {   // (ascending: the smallest L of the greatest weight stays)
      best = w120[i];
      m.mode = length[i];
    }
  }
  m.mean = to_double(u256_of(swl)) / (double)W;
  const U256 a = mul256_64(swl2, W), b = mul128(swl, swl);   // W sum w L^2 >= (sum w L)^2
  m.sd = cmp256(a, b) > 0 ? std::sqrt(to_double(sub256(a, b))) / (double)W : 0.0;
  // percentiles: the smallest L whose cumulative weight times 100 is >= q W
  const unsigned q[5] = {5, 25, 50, 75, 95};
  uint64_t* dst[5] = {&m.p5, &m.q25, &m.median, &m.q75, &m.p95};
  u128_t cum = 0;
  int at = 0;
  std::vector<u128_t> cls((size_t)n_cuts + 1, 0);
  for (size_t i = 0; i < n_classes; i++) {
    cum += w120[i];
    while (at < 5 && (u128_t)100 * cum >= (u128_t)q[at] * W) *dst[at++] = length[i];
    int k = 0;
    while (k < n_cuts && length[i] >= cuts[k]) k++;   // class k: cuts[k - 1] <= L < cuts[k]
    cls[(size_t)k] += w120[i];
  }
  for (int k = 0; k <= n_cuts; k++) m.share[k] = (double)(uint64_t)cls[(size_t)k] / (double)W;
  *out = m;
  return GX_OK;
}

// --lengths: one row per sample and occurring length, then the sample's inverted intervals, if any
int gx_format_lengths(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* const* length, const uint64_t* const* n,
                      const uint64_t* const* w120, const size_t* n_classes, const uint64_t* n_inverted, const uint64_t* w120_inverted, int cut_sites) {
  if (!out || n_samples < 1 || !rep || !is_ctrl || !length || !n || !w120 || !n_classes || !n_inverted || !w120_inverted) return GX_ERR_ORDER;
  std::vector<uint64_t> W((size_t)n_samples);
  for (int s = 0; s < n_samples; s++) {
    uint64_t N = 0;
    if (!len_classes_ok(length[s], n[s], w120[s], n_classes[s], &N, &W[s])) return GX_ERR_ORDER;
  }
  if (cut_sites)
    fprintf(out, "# an interval is a cut-site window of -j (ATAC mode), not a fragment: nearly all have one length; length = end (clamped to the chromosome) - start; weight = 1 / alignments\n");
  else
    fprintf(out, "# an interval is one of the sample's -b lines: a fragment, or an unpaired read as -y / -w extend it (with -j: cut-site windows instead); length = end (clamped to the chromosome) - start; weight = 1 / alignments\n");
  fprintf(out, "sample\tlength\tintervals\tweight\tcum_weight_share\n");
  for (int s = 0; s < n_samples; s++) {
    uint64_t cum = 0;
    for (size_t i = 0; i < n_classes[s]; i++) {
      cum += w120[s][i];
      fprintf(out, "%c%d\t%llu\t%llu", is_ctrl[s] ? 'c' : 't', rep[s], (unsigned long long)length[s][i], (unsigned long long)n[s][i]);
      put_w120(out, w120[s][i]);
      fprintf(out, "\t%.6f\n", (double)cum / (double)W[s]);
    }
    if (n_inverted[s]) {
      fprintf(out, "%c%d\tinverted\t%llu", is_ctrl[s] ? 'c' : 't', rep[s], (unsigned long long)n_inverted[s]);
      put_w120(out, w120_inverted[s]);
      fprintf(out, "\tNA\n");
    }
  }
  return GX_OK;
}

// --lengths-metrics: one row per sample
int gx_format_lengths_metrics(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* const* length, const uint64_t* const* n,
                              const uint64_t* const* w120, const size_t* n_classes, const uint64_t* cuts, int n_cuts) {
  if (!out || n_samples < 1 || !rep || !is_ctrl || !length || !n || !w120 || !n_classes) return GX_ERR_ORDER;
  std::vector<gx_len_metrics> m((size_t)n_samples);
  for (int s = 0; s < n_samples; s++)
    if (int rc = gx_lengths_metrics(length[s], n[s], w120[s], n_classes[s], cuts, n_cuts, &m[s])) return rc;
  fprintf(out, "sample\tintervals\tweight\tmean\tsd\tmin\tp5\tq25\tmedian\tq75\tp95\tmax\tmode");
  for (int k = 0; k <= n_cuts; k++) {
    if (k == 0 && n_cuts) fprintf(out, "\tlt%llu", (unsigned long long)cuts[0]);
    else if (k == 0) fprintf(out, "\tall");
    else if (k == n_cuts) fprintf(out, "\tge%llu", (unsigned long long)cuts[k - 1]);
    else fprintf(out, "\tge%llu_lt%llu", (unsigned long long)cuts[k - 1], (unsigned long long)cuts[k]);
  }
  fprintf(out, "\n");
  for (int s = 0; s < n_samples; s++) {
    fprintf(out, "%c%d\t%llu", is_ctrl[s] ? 'c' : 't', rep[s], (unsigned long long)m[s].n);
    put_w120(out, m[s].w120);
    put_cpx(out, m[s].mean, "\t%.6f");
    put_cpx(out, m[s].sd, "\t%.6f");
    for (uint64_t v : {m[s].min, m[s].p5, m[s].q25, m[s].median, m[s].q75, m[s].p95, m[s].max, m[s].mode}) fprintf(out, "\t%llu", (unsigned long long)v);
    for (int k = 0; k <= n_cuts; k++) fprintf(out, "\t%.6f", m[s].n ? m[s].share[k] : 0.0);
    fprintf(out, "\n");
  }
  return GX_OK;
}

// --chrom-stats: one row per chromosome of the table, four columns per sample
int gx_format_chrom_stats(FILE* out, const char* const* names, const uint32_t* lens, int n_chrom, int n_samples, const int* rep, const int* is_ctrl,
                          const uint64_t* const* cn, const uint64_t* const* cw120, const uint64_t* const* cbases120) {
  if (!out || !names || !lens || n_chrom < 1 || n_samples < 1 || !rep || !is_ctrl || !cn || !cw120 || !cbases120) return GX_ERR_ORDER;
  std::vector<u128_t> W((size_t)n_samples, 0);
  for (int s = 0; s < n_samples; s++) {
    if (!cn[s] || !cw120[s] || !cbases120[s]) return GX_ERR_ORDER;
    for (int c = 0; c < n_chrom; c++) W[s] += cw120[s][c];
    if (W[s] >> 64) return GX_ERR_ORDER;
  }
  fprintf(out, "# intervals, weight and share count every interval of the sample on the chromosome; mean_depth = sum of weight x length / chromosome length; a chromosome skipped with -e never reaches the library: its row is zeros\n");
  fprintf(out, "chrom\tlength");
  for (int s = 0; s < n_samples; s++) {
    char lab[32];
    snprintf(lab, sizeof lab, "%c%d", is_ctrl[s] ? 'c' : 't', rep[s]);
    fprintf(out, "\t%s.intervals\t%s.weight\t%s.share\t%s.mean_depth", lab, lab, lab, lab);
  }
  fprintf(out, "\n");
  for (int c = 0; c < n_chrom; c++) {
    fprintf(out, "%s\t%u", names[c], lens[c]);
    for (int s = 0; s < n_samples; s++) {
      fprintf(out, "\t%llu", (unsigned long long)cn[s][c]);
      put_w120(out, cw120[s][c]);
      fprintf(out, "\t%.6f\t%.6f", W[s] ? (double)cw120[s][c] / (double)(uint64_t)W[s] : 0.0,
              lens[c] ? (double)cbases120[s][c] / (double)(120ull * lens[c]) : 0.0);
    }
    fprintf(out, "\n");
  }
  return GX_OK;
}

// --xcor / --xcor-metrics: the curve and the figures from the integers alone
namespace {
bool xcor_counts_ok(uint64_t N, uint64_t nP, uint64_t nM, int lo, int hi, const uint64_t* n11) {
  if (lo < -GX_XCOR_MAX_SHIFT || hi > GX_XCOR_MAX_SHIFT || lo > hi || !n11 || nP > N || nM > N) return false;
  for (int d = lo; d <= hi; d++)
    if (n11[d - lo] > nP || n11[d - lo] > nM) return false;
  return true;
}
// r(d) for every shift: the numerator N n11 - nP nM (a signed 128-bit integer: both products lie below 2^128) and the radicand
// nP (N - nP) nM (N - nM) (256 bits) exact, each converted once (to_double), one square root, one division; NaN when the
// radicand is 0
void xcor_curve(uint64_t N, uint64_t nP, uint64_t nM, int lo, int hi, const uint64_t* n11, double* r) {
  const U256 rad = mul128((u128_t)nP * (N - nP), (u128_t)nM * (N - nM));
  const bool none = cmp256(rad, U256()) == 0;
  const double den = none ? 0.0 : std::sqrt(to_double(rad));
  const u128_t pm = (u128_t)nP * nM;
  for (int d = lo; d <= hi; d++) {
    if (none) {
      r[d - lo] = std::nan("");
      continue;
    }
    const u128_t a = (u128_t)N * n11[d - lo];
    const double num = a >= pm ? to_double(u256_of(a - pm)) : -to_double(u256_of(pm - a));
    r[d - lo] = num / den;
  }
}
}  // namespace

int gx_xcor_r(uint64_t n_pos, uint64_t n_plus, uint64_t n_minus, int lo, int hi, const uint64_t* n11, double* r) {
  if (!r || !xcor_counts_ok(n_pos, n_plus, n_minus, lo, hi, n11)) return GX_ERR_ORDER;
  xcor_curve(n_pos, n_plus, n_minus, lo, hi, n11, r);
  return GX_OK;
}

int gx_xcor_metrics(uint64_t n_pos, uint64_t n_plus, uint64_t n_minus, int lo, int hi, const uint64_t* n11, int read_len, gx_xcor_metrics_t* out) {
  if (!out || read_len < 0 || !xcor_counts_ok(n_pos, n_plus, n_minus, lo, hi, n11)) return GX_ERR_ORDER;
  std::vector<double> r((size_t)(hi - lo + 1));
  xcor_curve(n_pos, n_plus, n_minus, lo, hi, n11, r.data());
  gx_xcor_metrics_t m{};
  const double nan = std::nan("");
  m.r_frag = m.r_min = m.r_phantom = m.nsc = m.rsc = nan;
  const int ph = read_len - 1;
  m.phantom_shift = read_len ? ph : 0;
  m.has_phantom = read_len && ph >= lo && ph <= hi;
  if (m.has_phantom) m.r_phantom = r[(size_t)(ph - lo)];
  m.min_shift = lo;
  if (!std::isnan(r[0])) {   // (the radicand does not depend on d: all of r is NaN or none of it)
    m.r_min = r[0];
    for (int d = lo; d <= hi; d++) {
      const double v = r[(size_t)(d - lo)];
      if (v < m.r_min) {   // (ascending: the smallest d of the least r stays)
        m.r_min = v;
        m.min_shift = d;
      }
      if (d < 1 || (read_len && d >= ph - 10 && d <= ph + 10)) continue;
      if (!m.has_frag || v > m.r_frag) {
        m.has_frag = 1;
        m.r_frag = v;
        m.frag_shift = d;
      }
    }
  }
  if (m.has_frag) {
    m.fragment_length = m.frag_shift + 1;
    if (m.r_min > 0.0) m.nsc = m.r_frag / m.r_min;
    if (m.has_phantom && m.r_phantom - m.r_min > 0.0) m.rsc = (m.r_frag - m.r_min) / (m.r_phantom - m.r_min);
  }
  *out = m;
  return GX_OK;
}

// --xcor: one row per sample and shift under the sample's line of totals
int gx_format_xcor(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* n_pos, const uint64_t* n_plus,
                   const uint64_t* n_minus, const uint64_t* rejected, int lo, int hi, const uint64_t* const* n11) {
  if (!out || n_samples < 1 || !rep || !is_ctrl || !n_pos || !n_plus || !n_minus || !rejected || !n11) return GX_ERR_ORDER;
  for (int s = 0; s < n_samples; s++)
    if (!xcor_counts_ok(n_pos[s], n_plus[s], n_minus[s], lo, hi, n11[s])) return GX_ERR_ORDER;
  std::vector<double> r((size_t)(hi - lo + 1));
  fprintf(out, "sample\tshift\tn11\tr\n");
  for (int s = 0; s < n_samples; s++) {
    const char k = is_ctrl[s] ? 'c' : 't';
    fprintf(out, "# %c%d\tn_pos=%llu\tn_plus=%llu\tn_minus=%llu\trejected=%llu\n", k, rep[s], (unsigned long long)n_pos[s], (unsigned long long)n_plus[s],
            (unsigned long long)n_minus[s], (unsigned long long)rejected[s]);
    xcor_curve(n_pos[s], n_plus[s], n_minus[s], lo, hi, n11[s], r.data());
    for (int d = lo; d <= hi; d++) {
      fprintf(out, "%c%d\t%d\t%llu", k, rep[s], d, (unsigned long long)n11[s][d - lo]);
      put_cpx(out, r[(size_t)(d - lo)], "\t%.6f");
      fprintf(out, "\n");
    }
  }
  return GX_OK;
}

// --xcor-metrics: one row per sample
int gx_format_xcor_metrics(FILE* out, int n_samples, const int* rep, const int* is_ctrl, const uint64_t* n_pos, const uint64_t* n_plus,
                           const uint64_t* n_minus, int lo, int hi, const uint64_t* const* n11, int read_len) {
  if (!out || n_samples < 1 || !rep || !is_ctrl || !n_pos || !n_plus || !n_minus || !n11) return GX_ERR_ORDER;
  std::vector<gx_xcor_metrics_t> m((size_t)n_samples);
  for (int s = 0; s < n_samples; s++)
    if (int rc = gx_xcor_metrics(n_pos[s], n_plus[s], n_minus[s], lo, hi, n11[s], read_len, &m[s])) return rc;
  fprintf(out, "sample\tn_pos\tn_plus\tn_minus\tfragment_length\tr_frag\tmin_shift\tr_min\tphantom_shift\tr_phantom\tNSC\tRSC\n");
  for (int s = 0; s < n_samples; s++) {
    fprintf(out, "%c%d\t%llu\t%llu\t%llu", is_ctrl[s] ? 'c' : 't', rep[s], (unsigned long long)n_pos[s], (unsigned long long)n_plus[s],
            (unsigned long long)n_minus[s]);
    if (m[s].has_frag) fprintf(out, "\t%d", m[s].fragment_length);
    else fprintf(out, "\tNA");
    put_cpx(out, m[s].r_frag, "\t%.6f");
    if (std::isnan(m[s].r_min)) fprintf(out, "\tNA");
    else fprintf(out, "\t%d", m[s].min_shift);
    put_cpx(out, m[s].r_min, "\t%.6f");
    if (read_len) fprintf(out, "\t%d", m[s].phantom_shift);
    else fprintf(out, "\tNA");
    put_cpx(out, m[s].r_phantom, "\t%.6f");
    put_cpx(out, m[s].nsc, "\t%.6f");
    put_cpx(out, m[s].rsc, "\t%.6f");
    fprintf(out, "\n");
  }
  return GX_OK;
}

// --depth / --depth-metrics: the figures from the integers alone, every sum an exact big integer before anything is a double
namespace {
// what the formatters and the figures walk: (whole depth, bases) ascending, the depth-0 row first and always there (the bases at
// pileup 0 and class 0's), deep entries grouped by v div 120; false: the histogram contradicts itself
struct DepthRows {
  std::vector<uint64_t> depth, bases;
  uint64_t B = 0, covered = 0;
};
bool depth_rows(const gx_depth_hist& h, DepthRows& R) {
  if (!h.bases || !h.rsum || !h.rsq || (h.n_deep && (!h.deep_v || !h.deep_bases)) || h.excluded > h.total) return false;
  R.B = h.total - h.excluded;
  u128_t covered = 0;
  R.depth.assign(1, 0);
  R.bases.assign(1, h.bases[0]);
  covered += h.bases[0];
  for (uint32_t d = 0; d < GX_DEPTH_BOUND; d++) {
    if ((u128_t)h.rsum[d] > (u128_t)119 * h.bases[d] || (u128_t)h.rsq[d] > (u128_t)119 * h.rsum[d] || h.rsq[d] < h.rsum[d]) return false;
    if (d == 0 && h.bases[0] && !h.rsum[0]) return false;   // (class 0 holds 0 < v < 120 only)
    if (!d || !h.bases[d]) continue;
    R.depth.push_back(d);
    R.bases.push_back(h.bases[d]);
    covered += h.bases[d];
  }
  for (size_t i = 0; i < h.n_deep; i++) {
    if (h.deep_v[i] < (uint64_t)120 * GX_DEPTH_BOUND || !h.deep_bases[i] || (i && h.deep_v[i - 1] >= h.deep_v[i])) return false;
    const uint64_t d = h.deep_v[i] / 120;
    if (R.depth.back() == d) R.bases.back() += h.deep_bases[i];
    else {
      R.depth.push_back(d);
      R.bases.push_back(h.deep_bases[i]);
    }
    covered += h.deep_bases[i];
  }
  if (covered + h.zero != (u128_t)R.B) return false;
  R.covered = (uint64_t)covered;
  R.bases[0] += h.zero;
  if (R.covered && (!h.min_v || h.max_v < h.min_v)) return false;
  return true;
}
void put_depth_value(FILE* out, uint64_t v) {   // a pileup in 1/120 units, as --coverage prints a value
  if (v % 120 == 0) fprintf(out, "\t%llu", (unsigned long long)(v / 120));
  else fprintf(out, "\t%.4f", (double)v / 120.0);
}
const unsigned DEPTH_GE[GX_DEPTH_NGE] = {1, 2, 5, 10, 20, 50, 100};
}  // namespace

int gx_depth_metrics(const gx_depth_hist* hist, gx_depth_metrics_t* out) {
  DepthRows R;
  if (!hist || !out || !depth_rows(*hist, R)) return GX_ERR_ORDER;
  const gx_depth_hist& h = *hist;
  gx_depth_metrics_t m{};
  const double nan = std::nan("");
  m.bases = R.B;
  m.excluded = h.excluded;
  m.covered = R.covered;
  m.min_v = (h.zero || !R.covered) ? 0 : h.min_v;
  m.max_v = R.covered ? h.max_v : 0;
  // sum v and sum v^2 over the bases, exact
  U256 sv, sv2;
  for (uint32_t d = 0; d < GX_DEPTH_BOUND; d++) {
    if (!h.bases[d]) continue;
    sv = add256(sv, u256_of((u128_t)(120ull * d) * h.bases[d] + h.rsum[d]));
    sv2 = add256(sv2, u256_of((u128_t)(14400ull * d * d) * h.bases[d]));
    sv2 = add256(sv2, u256_of((u128_t)(240ull * d) * h.rsum[d] + h.rsq[d]));
  }
  for (size_t i = 0; i < h.n_deep; i++) {
    sv = add256(sv, u256_of((u128_t)h.deep_v[i] * h.deep_bases[i]));
    sv2 = add256(sv2, mul128((u128_t)h.deep_v[i] * h.deep_v[i], h.deep_bases[i]));
  }
  const u128_t sv128 = ((u128_t)sv.w[1] << 64) | sv.w[0];   // (sum v < 2^64 * 2^64: deep_v is checked against nothing above, so ...)
  if (sv.w[2] | sv.w[3]) return GX_ERR_ORDER;              // (... a made-up list beyond it is refused)
  if (R.B) {
    const double nb = 120.0 * (double)R.B;
    m.covered_fraction = (double)R.covered / (double)R.B;
    m.mean = to_double(sv) / nb;
    const U256 a = mul256_64(sv2, R.B), b = mul128(sv128, sv128);   // B sum v^2 >= (sum v)^2
    if (sv2.w[3] || cmp256(a, b) < 0) return GX_ERR_ORDER;
    m.sd = std::sqrt(to_double(sub256(a, b))) / nb;
  } else {
    m.mean = m.sd = nan;
  }
  // percentiles: the smallest whole depth d with 100 #(bases of depth <= d) >= q B
  const unsigned q[5] = {25, 50, 75, 95, 99};
  uint64_t* dst[5] = {&m.q25, &m.median, &m.q75, &m.p95, &m.p99};
  u128_t below = 0;
  int at = 0;
  for (size_t i = 0; i < R.depth.size() && at < 5; i++) {
    below += R.bases[i];
    while (at < 5 && (u128_t)100 * below >= (u128_t)q[at] * R.B) *dst[at++] = R.depth[i];
  }
  for (int k = 0; k < GX_DEPTH_NGE; k++) {
    u128_t n = 0;
    for (size_t i = 0; i < R.depth.size(); i++)
      if (R.depth[i] >= DEPTH_GE[k]) n += R.bases[i];
    m.ge[k] = R.B ? (double)(uint64_t)n / (double)R.B : 0.0;
  }
  *out = m;
  return GX_OK;
}

// --depth: one row per sample and non-empty whole depth
int gx_format_depth(FILE* out, int n_samples, const gx_depth_hist* hist) {
  if (!out || n_samples < 1 || !hist) return GX_ERR_ORDER;
  std::vector<DepthRows> R((size_t)n_samples);
  for (int s = 0; s < n_samples; s++)
    if (!depth_rows(hist[s], R[s])) return GX_ERR_ORDER;
  fprintf(out, "#sample\tdepth\tbases\tbases_at_least\tfraction_at_least\n");
  for (int s = 0; s < n_samples; s++) {
    uint64_t atLeast = R[s].B;
    for (size_t i = 0; i < R[s].depth.size(); i++) {
      fprintf(out, "%c%d\t%llu\t%llu\t%llu\t%.6f\n", hist[s].is_ctrl ? 'c' : 't', (int)hist[s].rep, (unsigned long long)R[s].depth[i],
              (unsigned long long)R[s].bases[i], (unsigned long long)atLeast, R[s].B ? (double)atLeast / (double)R[s].B : 0.0);
      atLeast -= R[s].bases[i];
    }
  }
  return GX_OK;
}

// --depth-metrics: one row per sample
int gx_format_depth_metrics(FILE* out, int n_samples, const gx_depth_hist* hist) {
  if (!out || n_samples < 1 || !hist) return GX_ERR_ORDER;
  std::vector<gx_depth_metrics_t> m((size_t)n_samples);
  for (int s = 0; s < n_samples; s++)
    if (int rc = gx_depth_metrics(&hist[s], &m[s])) return rc;
  fprintf(out, "sample\tbases\texcluded\tcovered\tcovered_fraction\tmean\tsd\tmin\tq25\tmedian\tq75\tp95\tp99\tmax");
  for (int k = 0; k < GX_DEPTH_NGE; k++) fprintf(out, "\tge%u", DEPTH_GE[k]);
  fprintf(out, "\n");
  for (int s = 0; s < n_samples; s++) {
    fprintf(out, "%c%d\t%llu\t%llu\t%llu\t%.6f", hist[s].is_ctrl ? 'c' : 't', (int)hist[s].rep, (unsigned long long)m[s].bases,
            (unsigned long long)m[s].excluded, (unsigned long long)m[s].covered, m[s].covered_fraction);
    put_cpx(out, m[s].mean, "\t%.6f");
    put_cpx(out, m[s].sd, "\t%.6f");
    put_depth_value(out, m[s].min_v);
    fprintf(out, "\t%llu\t%llu\t%llu\t%llu\t%llu", (unsigned long long)m[s].q25, (unsigned long long)m[s].median, (unsigned long long)m[s].q75,
            (unsigned long long)m[s].p95, (unsigned long long)m[s].p99);
    put_depth_value(out, m[s].max_v);
    for (int k = 0; k < GX_DEPTH_NGE; k++) fprintf(out, "\t%.6f", m[s].ge[k]);
    fprintf(out, "\n");
  }
  return GX_OK;
}

// --saturation: two peak lists in gx_get_peaks order, one merge walk (the --counts predicate: s < pe && ps < e)
int gx_saturation_overlap(const gx_peak* full, size_t n_full, const gx_peak* sub, size_t n_sub, uint64_t* full_recovered,
                          uint64_t* sub_in_full, uint64_t* shared_bp) {
  if ((n_full && !full) || (n_sub && !sub)) return GX_ERR_ORDER;
  uint64_t rec = 0, in = 0, bp = 0;
  size_t i = 0, j = 0, lastI = (size_t)-1, lastJ = (size_t)-1;
  while (i < n_full && j < n_sub) {
    const gx_peak &F = full[i], &S = sub[j];
    if (F.chrom != S.chrom) {
      (F.chrom < S.chrom ? i : j)++;
    } else if (F.end <= S.start) {
      i++;
    } else if (S.end <= F.start) {
      j++;
    } else {
      if (i != lastI) rec++;
      if (j != lastJ) in++;
      lastI = i;
      lastJ = j;
      bp += std::min(F.end, S.end) - std::max(F.start, S.start);
      if (F.end <= S.end) i++;   // (whichever ends first cannot touch what follows in the other list)
      else j++;
    }
  }
  if (full_recovered) *full_recovered = rec;
  if (sub_in_full) *sub_in_full = in;
  if (shared_bp) *shared_bp = bp;
  return GX_OK;
}

int gx_saturation_thresholds(int n_points, uint64_t* threshold) {
  if (n_points < 1 || n_points > 100 || !threshold) return GX_ERR_ORDER;
  for (int j = 1; j <= n_points; j++) threshold[j - 1] = ((uint64_t)j << 32) / (uint64_t)n_points;
  return GX_OK;
}

// ... one row per point, under a comment line with the run's own peaks
int gx_format_saturation(FILE* out, int n_points, const gx_sat_point* points, const uint64_t* full_recovered, const uint64_t* sub_in_full,
                         const uint64_t* shared_bp, uint64_t n_full, uint64_t full_bp) {
  if (!out || n_points < 1 || !points || !full_recovered || !sub_in_full || !shared_bp) return GX_ERR_ORDER;
  fprintf(out, "# run: %llu peaks, %llu bp\n", (unsigned long long)n_full, (unsigned long long)full_bp);
  fprintf(out, "fraction\tthreshold\tkept\tpeaks\tpeak_bp\trecovered\trecovered_share\tin_run\tshared_bp\tstatus\n");
  for (int j = 0; j < n_points; j++) {
    const gx_sat_point& p = points[j];
    fprintf(out, "%.6f\t%llu\t%llu\t%llu\t%llu\t%llu", (double)p.threshold / 4294967296.0, (unsigned long long)p.threshold,
            (unsigned long long)p.n_kept, (unsigned long long)p.n_peaks, (unsigned long long)p.peak_bp, (unsigned long long)full_recovered[j]);
    if (n_full) fprintf(out, "\t%.6f", (double)full_recovered[j] / (double)n_full);
    else fprintf(out, "\tNA");
    fprintf(out, "\t%llu\t%llu", (unsigned long long)sub_in_full[j], (unsigned long long)shared_bp[j]);
    if (p.status == GX_OK) fprintf(out, "\tok\n");
    else if (p.status == GX_ERR_EXPT) fprintf(out, "\tno_fragments\n");
    else fprintf(out, "\t%d\n", (int)p.status);
  }
  return GX_OK;
}

// --reproducibility: which peaks of `a` a peak of `b` supports; two lists in gx_get_peaks order, one merge walk over the
// overlapping pairs (whichever peak ends first cannot overlap what follows in the other list)
int gx_peaks_supported(const gx_peak* a, size_t n_a, const gx_peak* b, size_t n_b, int pct, uint8_t* hit) {
  if ((n_a && (!a || !hit)) || (n_b && !b) || pct < 0 || pct > 100) return GX_ERR_ORDER;
  for (size_t i = 0; i < n_a; i++) hit[i] = 0;
  size_t i = 0, j = 0;
  while (i < n_a && j < n_b) {
    const gx_peak &A = a[i], &B = b[j];
    if (A.chrom != B.chrom) {
      (A.chrom < B.chrom ? i : j)++;
    } else if (A.end <= B.start) {
      i++;
    } else if (B.end <= A.start) {
      j++;
    } else {
      const uint64_t ov = (uint64_t)std::min(A.end, B.end) - (uint64_t)std::max(A.start, B.start);
      const uint64_t shorter = std::min((uint64_t)A.end - A.start, (uint64_t)B.end - B.start);
      if (100 * ov >= (uint64_t)pct * shorter) hit[i] = 1;
      if (A.end <= B.end) i++;
      else j++;
    }
  }
  return GX_OK;
}

// ... and the figures made of it.  The calls are gx_reproducibility's, in its order: ALONE r at r, SELF r h at R + 2 r + h,
// POOLED h at 3 R + h.
int gx_reproducibility_figures(const gx_peak* run, size_t n_run, int n_rep, const gx_repro_call* calls, const gx_peak* const* peaks, int pct,
                               gx_repro_figures* fig, uint64_t* nt_pair, uint64_t* n_self, uint64_t* in_run, uint64_t* run_supported,
                               uint8_t* conservative, uint8_t* optimal) {
  if (n_rep < 1 || !calls || !peaks || !fig || (n_run && !run) || pct < 0 || pct > 100 || !n_self || (n_rep > 1 && !nt_pair)) return GX_ERR_ORDER;
  const int R = n_rep, nC = 3 * R + 2;
  for (int i = 0; i < nC; i++) {
    const gx_repro_call& c = calls[i];
    const bool ok = i < R ? c.kind == GX_REPRO_ALONE && c.rep == i
                    : i < 3 * R ? c.kind == GX_REPRO_SELF && c.rep == (i - R) / 2 && c.half == (i - R) % 2
                                : c.kind == GX_REPRO_POOLED && c.half == i - 3 * R;
    if (!ok || (c.n_peaks && !peaks[i])) return GX_ERR_ORDER;
  }
  // the run's peaks against every call, and every call's against the run's
  std::vector<std::vector<uint8_t>> sup((size_t)nC, std::vector<uint8_t>(n_run, 0));
  std::vector<uint8_t> tmp;
  for (int i = 0; i < nC; i++) {
    const size_t n = (size_t)calls[i].n_peaks;
    if (int rc = gx_peaks_supported(run, n_run, peaks[i], n, pct, sup[i].data())) return rc;
    tmp.assign(n, 0);
    if (int rc = gx_peaks_supported(peaks[i], n, run, n_run, pct, tmp.data())) return rc;
    if (run_supported) run_supported[i] = (uint64_t)std::count(sup[i].begin(), sup[i].end(), 1);
    if (in_run) in_run[i] = (uint64_t)std::count(tmp.begin(), tmp.end(), 1);
  }
  auto both = [&](int x, int y) {
    uint64_t n = 0;
    for (size_t k = 0; k < n_run; k++) n += sup[x][k] & sup[y][k];
    return n;
  };
  *fig = gx_repro_figures{};
  fig->n_rep = R;
  fig->best_i = fig->best_j = -1;
  for (int i = 0, at = 0; i < R; i++)
    for (int j = i + 1; j < R; j++, at++) {
      nt_pair[at] = both(i, j);
      if (fig->best_i < 0 || nt_pair[at] > fig->nt) {   // (a tie: the first pair)
        fig->nt = nt_pair[at];
        fig->best_i = i;
        fig->best_j = j;
      }
    }
  fig->np = both(3 * R, 3 * R + 1);
  for (int r = 0; r < R; r++) {   // ALONE r's peaks that both of its halves support
    const size_t n = (size_t)calls[r].n_peaks;
    std::vector<uint8_t> h0(n, 0), h1(n, 0);
    for (int h = 0; h < 2; h++)
      if (int rc = gx_peaks_supported(peaks[r], n, peaks[R + 2 * r + h], (size_t)calls[R + 2 * r + h].n_peaks, pct, (h ? h1 : h0).data())) return rc;
    n_self[r] = 0;
    for (size_t k = 0; k < n; k++) n_self[r] += h0[k] & h1[k];
    fig->n_self_max = r ? std::max(fig->n_self_max, n_self[r]) : n_self[r];
    fig->n_self_min = r ? std::min(fig->n_self_min, n_self[r]) : n_self[r];
  }
  const uint64_t hi = std::max(fig->np, fig->nt), lo = std::min(fig->np, fig->nt);
  fig->rescue_na = R == 1 || lo == 0;
  fig->self_na = R == 1 || fig->n_self_min == 0;
  fig->rescue = fig->rescue_na ? 0.0 : (double)hi / (double)lo;
  fig->self_consistency = fig->self_na ? 0.0 : (double)fig->n_self_max / (double)fig->n_self_min;
  if (fig->rescue_na || fig->self_na)
    fig->verdict = GX_REPRO_NA;
  else {
    const int good = (hi < 2 * lo) + (fig->n_self_max < 2 * fig->n_self_min);
    fig->verdict = good == 2 ? GX_REPRO_PASS : good == 1 ? GX_REPRO_BORDERLINE : GX_REPRO_FAIL;
  }
  // the sets: the run's peaks counted in Nt, and the larger of those and Np's (a tie: the conservative set)
  fig->n_conservative = R > 1 ? fig->nt : 0;
  fig->optimal_is_pooled = fig->np > fig->n_conservative;
  fig->n_optimal = std::max(fig->np, fig->n_conservative);
  for (size_t k = 0; k < n_run; k++) {
    const uint8_t cons = R > 1 ? sup[fig->best_i][k] & sup[fig->best_j][k] : 0, pool = sup[3 * R][k] & sup[3 * R + 1][k];
    if (conservative) conservative[k] = cons;
    if (optimal) optimal[k] = fig->optimal_is_pooled ? pool : cons;
  }
  return GX_OK;
}

static std::string repro_label(const gx_repro_call& c) {
  if (c.kind == GX_REPRO_POOLED) return "pooled.pr" + std::to_string(c.half + 1);
  std::string s = "t" + std::to_string(c.rep + 1);
  return c.kind == GX_REPRO_SELF ? s + ".pr" + std::to_string(c.half + 1) : s;
}

int gx_reproducibility_label(const gx_repro_call* call, char* out, size_t cap) {
  if (!call || !out || !cap) return GX_ERR_ORDER;
  snprintf(out, cap, "%s", repro_label(*call).c_str());
  return GX_OK;
}

// ... one row per call, under a comment line with the run's own peaks, the overlap asked for and the seed
int gx_format_reproducibility(FILE* out, int n_rep, const gx_repro_call* calls, const uint64_t* in_run, const uint64_t* run_supported,
                              uint64_t n_run, uint64_t run_bp, int pct, uint64_t seed) {
  if (!out || n_rep < 1 || !calls || !in_run || !run_supported) return GX_ERR_ORDER;
  fprintf(out, "# run: %llu peaks, %llu bp; overlap %d %%; seed %llu\n", (unsigned long long)n_run, (unsigned long long)run_bp, pct,
          (unsigned long long)seed);
  fprintf(out, "call\trep\thalf\tintervals\tpeaks\tpeak_bp\tin_run\trun_supported\tstatus\n");
  for (int i = 0; i < 3 * n_rep + 2; i++) {
    const gx_repro_call& c = calls[i];
    fprintf(out, "%s", repro_label(c).c_str());
    if (c.rep < 0) fprintf(out, "\tNA");
    else fprintf(out, "\t%d", c.rep + 1);
    if (c.half < 0) fprintf(out, "\tNA");
    else fprintf(out, "\t%d", c.half + 1);
    fprintf(out, "\t%llu\t%llu\t%llu\t%llu\t%llu", (unsigned long long)c.n_events, (unsigned long long)c.n_peaks, (unsigned long long)c.peak_bp,
            (unsigned long long)in_run[i], (unsigned long long)run_supported[i]);
    if (c.status == GX_OK) fprintf(out, "\tok\n");
    else if (c.status == GX_ERR_EXPT) fprintf(out, "\tno_fragments\n");
    else fprintf(out, "\t%d\n", (int)c.status);
  }
  return GX_OK;
}

int gx_format_reproducibility_metrics(FILE* out, const gx_repro_figures* fig, const uint64_t* nt_pair, const uint64_t* n_self) {
  if (!out || !fig || fig->n_rep < 1 || !n_self || (fig->n_rep > 1 && !nt_pair)) return GX_ERR_ORDER;
  static const char* const verdict[] = {"pass", "borderline", "fail", "NA"};
  const int R = fig->n_rep;
  fprintf(out, "figure\tvalue\n");
  fprintf(out, "replicates\t%d\n", R);
  for (int i = 0, at = 0; i < R; i++)
    for (int j = i + 1; j < R; j++, at++) fprintf(out, "Nt.t%d.t%d\t%llu\n", i + 1, j + 1, (unsigned long long)nt_pair[at]);
  if (R > 1) fprintf(out, "Nt\t%llu\n", (unsigned long long)fig->nt);
  else fprintf(out, "Nt\tNA\n");
  fprintf(out, "Np\t%llu\n", (unsigned long long)fig->np);
  for (int r = 0; r < R; r++) fprintf(out, "N_self.t%d\t%llu\n", r + 1, (unsigned long long)n_self[r]);
  if (fig->rescue_na) fprintf(out, "rescue_ratio\tNA\n");
  else fprintf(out, "rescue_ratio\t%.6f\n", fig->rescue);
  if (fig->self_na) fprintf(out, "self_consistency_ratio\tNA\n");
  else fprintf(out, "self_consistency_ratio\t%.6f\n", fig->self_consistency);
  fprintf(out, "verdict\t%s\n", verdict[fig->verdict >= 0 && fig->verdict <= 3 ? fig->verdict : 3]);
  if (R > 1) fprintf(out, "conservative_peaks\t%llu\n", (unsigned long long)fig->n_conservative);
  else fprintf(out, "conservative_peaks\tNA\n");
  fprintf(out, "optimal_peaks\t%llu\n", (unsigned long long)fig->n_optimal);
  return GX_OK;
}

// -f after gx_find_peaks.  n_rep = number of replicates; peaks_opt = 0 for -X (logIntervals 837).
// thr / qval_opt as given to gx_create.
int gx_write_log_group(gx_ctx* const* ctxs, const int* owner, int n_rep, const char* const* names, int n_chrom, int qval_opt,
                       int peaks_opt, float thr, FILE* out) {
  const bool multi = n_rep > 1;
  if (multi) {
    fprintf(out, "chr\tstart\tend");
    for (int i = 0; i < n_rep; i++) fprintf(out, "\t-log(p)_%d", i);
    fprintf(out, "\t-log(p)_comb");
  } else
    fprintf(out, "chr\tstart\tend\texperimental\tcontrol\t-log(p)");
  if (qval_opt) fprintf(out, "\t-log(q)");
  if (peaks_opt) fprintf(out, "\tsignif");
  fprintf(out, "\n");
  Iv fin;
  std::vector<Iv> reps(multi ? n_rep : 0);
  for (int c = 0; c < n_chrom; c++) {
    gx_ctx* ctx = ctxs[owner ? owner[c] : 0];
    int rc = fetch(ctx, GX_IV_FINAL, c, fin, !multi, qval_opt != 0);
    if (rc) return rc;
    if (!fin.n) continue;
    std::vector<size_t> idx(multi ? n_rep : 0, 0);
    for (int r = 0; multi && r < n_rep; r++)
      if ((rc = fetch(ctx, r, c, reps[r], false, false))) return rc;
    uint32_t start = 0;
    for (size_t m = 0; m < fin.n; m++) {
      const float pv = fin.p[m], qv = qval_opt ? fin.q[m] : GX_SKIP;
      const float pq = qval_opt ? qv : pv;
      const bool sig = peaks_opt && pq > thr;  // callPeaks 1015
      if (!multi) {
        if (fin.ctrl[m] == GX_SKIP) {
          fprintf(out, "%s\t%d\t%d\t%f\t%f\t%s", names[c], start, fin.end[m], fin.expt[m], 0.0f, "NA");
          if (qval_opt) fprintf(out, "\t%s", "NA");
          fprintf(out, "\n");
        } else {
          fprintf(out, "%s\t%d\t%d\t%f\t%f\t%f", names[c], start, fin.end[m], fin.expt[m], fin.ctrl[m], pv);
          if (qval_opt) fprintf(out, "\t%f", qv);
          fprintf(out, "%s\n", sig ? "\t*" : "");
        }
      } else {
        fprintf(out, "%s\t%d\t%d", names[c], start, fin.end[m]);
        for (int r = 0; r < n_rep; r++)
          if (!reps[r].n || reps[r].p[idx[r]] == GX_SKIP)
            fprintf(out, "\t%s", "NA");
          else
            fprintf(out, "\t%f", reps[r].p[idx[r]]);
        if (pv == GX_SKIP) {
          fprintf(out, "\t%s", "NA");
          if (qval_opt) fprintf(out, "\t%s", "NA");
        } else {
          fprintf(out, "\t%f", pv);
          if (qval_opt) fprintf(out, "\t%f", qv);
        }
        fprintf(out, "%s\n", sig ? "\t*" : "");
        for (int r = 0; r < n_rep; r++)  // printLog 826-829
          if (reps[r].n && reps[r].end[idx[r]] == fin.end[m]) idx[r]++;
      }
      start = fin.end[m];
    }
  }
  return GX_OK;
}

// path-taking conveniences for FFI callers without a FILE*
int gx_write_log(gx_ctx* ctx, int n_rep, const char* const* names, int n_chrom, int qval_opt, int peaks_opt, float thr,
                 FILE* out) {
  return gx_write_log_group(&ctx, nullptr, n_rep, names, n_chrom, qval_opt, peaks_opt, thr, out);
}

int gx_write_narrowpeak_path(gx_ctx* ctx, const char* const* names, const char* path) {
  FILE* f = fopen(path, "w");
  if (!f) return GX_ERR_ORDER;
  int rc = gx_write_narrowpeak(ctx, names, f);
  fclose(f);
  return rc;
}
int gx_write_counts_path(gx_ctx* ctx, const char* const* names, int n_samples, const char* const* sample_names,
                         const char* path) {
  FILE* f = fopen(path, "w");
  if (!f) return GX_ERR_ORDER;
  int rc = gx_write_counts(ctx, names, n_samples, sample_names, f);
  fclose(f);
  return rc;
}
int gx_write_region_counts_path(gx_ctx* ctx, const char* const* names, const gx_region* regions, const char* const* region_names,
                                size_t n, int n_samples, const char* const* sample_names, const char* path) {
  FILE* f = fopen(path, "w");
  if (!f) return GX_ERR_ORDER;
  int rc = gx_write_region_counts(ctx, names, regions, region_names, n, n_samples, sample_names, f);
  fclose(f);
  return rc;
}
int gx_write_pile_path(gx_ctx* ctx, int rep, const char* const* names, int n_chrom, const char* expt_name,
                       const char* ctrl_name, const char* path, int append) {
  FILE* f = fopen(path, append ? "a" : "w");
  if (!f) return GX_ERR_ORDER;
  int rc = gx_write_pile(ctx, rep, names, n_chrom, expt_name, ctrl_name, f);
  fclose(f);
  return rc;
}
int gx_write_coverage_path(gx_ctx* ctx, int sample, const char* const* names, int n_chrom, double scale, const char* path) {
  FILE* f = fopen(path, "w");
  if (!f) return GX_ERR_ORDER;
  int rc = gx_write_coverage(ctx, sample, names, n_chrom, scale, f);
  fclose(f);
  return rc;
}
int gx_write_log_path(gx_ctx* ctx, int n_rep, const char* const* names, int n_chrom, int qval_opt, int peaks_opt,
                      float thr, const char* path) {
  FILE* f = fopen(path, "w");
  if (!f) return GX_ERR_ORDER;
  int rc = gx_write_log(ctx, n_rep, names, n_chrom, qval_opt, peaks_opt, thr, f);
  fclose(f);
  return rc;
}

// --gc-bias (no Genrich counterpart): the window classes folded into 101 percent classes, k = (200 g + W) / (2 W) in integers
// (halves up); per class ratio = (Nw[k] / sum Nw) / (F[k] / sum F) = double(Nw[k] * sum F) / double(F[k] * sum Nw), both
// products exact (128 bits), each converted once (to_double); NaN where F[k] or sum Nw is 0.  Host only.
int gx_gc_class(int window, int g) {
  if (window < 1 || window > GX_GC_MAX_WINDOW || g < 0 || g > window) return -1;
  return (200 * g + window) / (2 * window);
}

int gx_gc_metrics(int window, const uint64_t* F, uint64_t f_unclassed, const uint64_t* Nn, const uint64_t* Nw, uint64_t n_unclassed,
                  uint64_t w_unclassed, gx_gc_metrics_t* out) {
  if (!out || !F || !Nn || !Nw || window < 1 || window > GX_GC_MAX_WINDOW) return GX_ERR_ORDER;
  gx_gc_metrics_t m{};
  const double nan = std::nan("");
  u128_t sF = 0, sN = 0, sW = 0, gF = 0, gW = 0;
  for (int g = 0; g <= window; g++) {
    if (Nw[g] < Nn[g] || (u128_t)Nw[g] > (u128_t)120 * Nn[g]) return GX_ERR_ORDER;   // (every interval weighs between 1/120 and 1)
    const int k = gx_gc_class(window, g);
    m.cls_windows[k] += F[g];
    m.cls_intervals[k] += Nn[g];
    m.cls_w120[k] += Nw[g];
    sF += F[g];
    sN += Nn[g];
    sW += Nw[g];
    gF += (u128_t)F[g] * (unsigned)g;
    gW += (u128_t)Nw[g] * (unsigned)g;
  }
  if ((sF >> 64) || (sN >> 64) || (sW >> 64)) return GX_ERR_ORDER;
  m.windows = (uint64_t)sF;
  m.windows_unclassed = f_unclassed;
  m.intervals = (uint64_t)sN;
  m.intervals_unclassed = n_unclassed;
  m.w120 = (uint64_t)sW;
  m.w120_unclassed = w_unclassed;
  m.mean_gc_genome = sF ? to_double(u256_of(gF)) / to_double(u256_of(sF * (unsigned)window)) : nan;
  m.mean_gc_sample = sW ? to_double(u256_of(gW)) / to_double(u256_of(sW * (unsigned)window)) : nan;
  m.ratio_min = m.ratio_max = nan;
  m.ratio_min_class = m.ratio_max_class = -1;
  for (int k = 0; k < GX_GC_CLASSES; k++) {
    m.ratio[k] = nan;
    if (!m.cls_windows[k] || !sW) continue;
    m.ratio[k] = to_double(u256_of((u128_t)m.cls_w120[k] * sF)) / to_double(u256_of((u128_t)m.cls_windows[k] * sW));
    if ((u128_t)100 * m.cls_windows[k] < sF) continue;   // (the extremes: among the classes that hold 1 % of the windows)
    if (m.ratio_min_class < 0 || m.ratio[k] < m.ratio_min) {   // (ascending: the lowest class of the least ratio stays)
      m.ratio_min = m.ratio[k];
      m.ratio_min_class = k;
    }
    if (m.ratio_max_class < 0 || m.ratio[k] > m.ratio_max) {
      m.ratio_max = m.ratio[k];
      m.ratio_max_class = k;
    }
  }
  *out = m;
  return GX_OK;
}

// --gc-bias: one `#` line per sample, then its 101 rows
int gx_format_gc_bias(FILE* out, int n_samples, const int* rep, const int* is_ctrl, int window, const uint64_t* const* F, const uint64_t* f_unclassed,
                      const uint64_t* const* Nn, const uint64_t* const* Nw, const uint64_t* n_unclassed, const uint64_t* w_unclassed) {
  if (!out || n_samples < 1 || !rep || !is_ctrl || !F || !f_unclassed || !Nn || !Nw || !n_unclassed || !w_unclassed) return GX_ERR_ORDER;
  std::vector<gx_gc_metrics_t> m((size_t)n_samples);
  for (int s = 0; s < n_samples; s++)
    if (int rc = gx_gc_metrics(window, F[s], f_unclassed[s], Nn[s], Nw[s], n_unclassed[s], w_unclassed[s], &m[s])) return rc;
  fprintf(out, "sample\tgc_percent\twindows\tintervals\tweight\tratio\n");
  for (int s = 0; s < n_samples; s++) {
    const char k = is_ctrl[s] ? 'c' : 't';
    fprintf(out, "# %c%d\tW=%d\twindows=%llu\twindows_unclassed=%llu\tintervals=%llu\tintervals_unclassed=%llu\n", k, rep[s], window,
            (unsigned long long)m[s].windows, (unsigned long long)m[s].windows_unclassed, (unsigned long long)m[s].intervals,
            (unsigned long long)m[s].intervals_unclassed);
    for (int c = 0; c < GX_GC_CLASSES; c++) {
      fprintf(out, "%c%d\t%d\t%llu\t%llu", k, rep[s], c, (unsigned long long)m[s].cls_windows[c], (unsigned long long)m[s].cls_intervals[c]);
      put_w120(out, m[s].cls_w120[c]);
      put_cpx(out, m[s].ratio[c], "\t%.6f");
      fprintf(out, "\n");
    }
  }
  return GX_OK;
}

// --gc-peaks: the rows of --counts -- chr, start, end, peak_N in the order given -- then length, acgt, gc and gc / acgt
int gx_format_gc_peaks(FILE* out, const char* const* names, const gx_region* peaks, size_t n_peaks, const uint64_t* gc, const uint64_t* acgt) {
  if (!out || (n_peaks && (!peaks || !names || !gc || !acgt))) return GX_ERR_ORDER;
  for (size_t i = 0; i < n_peaks; i++)
    if (gc[i] > acgt[i] || peaks[i].end < peaks[i].start || acgt[i] > peaks[i].end - peaks[i].start) return GX_ERR_ORDER;
  fprintf(out, "chr\tstart\tend\tname\tlength\tacgt\tgc\tgc_fraction\n");
  for (size_t i = 0; i < n_peaks; i++) {
    const gx_region& k = peaks[i];
    fprintf(out, "%s\t%ld\t%ld\tpeak_%d\t%ld\t%llu\t%llu", names[k.chrom], (long)k.start, (long)k.end, (int)i, (long)k.end - (long)k.start,
            (unsigned long long)acgt[i], (unsigned long long)gc[i]);
    put_cpx(out, acgt[i] ? (double)gc[i] / (double)acgt[i] : std::nan(""), "\t%.6f");
    fprintf(out, "\n");
  }
  return GX_OK;
}

// --motifs (no Genrich counterpart): from a count matrix to scores in 1/128 bit against a uniform background and to the
// threshold of a p-value, counted exactly over all 4^L L-mers.  Host only.
static int motif_refuse(char* why, size_t cap, const char* text) {
  if (why && cap) snprintf(why, cap, "%s", text);
  return GX_ERR_ORDER;
}

int gx_motif_pssm(const uint32_t* counts, int width, double pseudocount, int16_t* scores, int32_t* smin, int32_t* smax, char* why, size_t cap) {
  if (width < 1 || width > GX_MOTIF_MAX_WIDTH) return motif_refuse(why, cap, "the width must satisfy 1 <= L <= 32");
  if (!counts || !scores) return GX_ERR_ORDER;
  if (!(pseudocount >= 0.0) || !std::isfinite(pseudocount)) return motif_refuse(why, cap, "the pseudocount must be a number >= 0");
  long long lo = 0, hi = 0;
  for (int j = 0; j < width; j++) {
    uint64_t N = 0;
    for (int b = 0; b < 4; b++) {
      if (counts[b * width + j] >> 31) return motif_refuse(why, cap, "a count of 2^31 or more");
      N += counts[b * width + j];
    }
    long long cmin = 0, cmax = 0;
    for (int b = 0; b < 4; b++) {
      const double num = (double)counts[b * width + j] + 0.25 * pseudocount, den = (double)N + pseudocount;
      if (!(den > 0.0) || !(num > 0.0)) return motif_refuse(why, cap, "a zero count without a pseudocount: the score would be minus infinity");
      const double v = 128.0 * std::log2((num / den) / 0.25);
      if (!(v > -40000.0 && v < 40000.0)) return motif_refuse(why, cap, "a score outside int16");
      const long long s = std::llround(v);
      if (s < -32768 || s > 32767) return motif_refuse(why, cap, "a score outside int16");
      scores[4 * j + b] = (int16_t)s;
      cmin = b ? std::min(cmin, s) : s;
      cmax = b ? std::max(cmax, s) : s;
    }
    lo += cmin;
    hi += cmax;
  }
  if (smin) *smin = (int32_t)lo;
  if (smax) *smax = (int32_t)hi;
  return GX_OK;
}

int gx_motif_threshold(const int16_t* scores, int width, double p, int32_t* threshold, int32_t* smin, int32_t* smax, double* p_achieved,
                       int* unreachable) {
  if (!scores || width < 1 || width > GX_MOTIF_MAX_WIDTH || !(p > 0.0) || !(p <= 1.0)) return GX_ERR_ORDER;
  // K = floor(p * 4^L): p = M * 2^(e - 53) with a 53-bit integer M
  int e = 0;
  const uint64_t M = (uint64_t)std::ldexp(std::frexp(p, &e), 53);
  const int sh = e - 53 + 2 * width;   // (at most 1 - 53 + 64)
  const u128_t K = sh >= 0 ? (u128_t)M << sh : sh > -64 ? (u128_t)(M >> -sh) : (u128_t)0;
  // dist[s - lo] = the L-mers of the columns so far whose score is s
  long long lo = 0, hi = 0;
  std::vector<u128_t> dist(1, (u128_t)1), next;
  for (int j = 0; j < width; j++) {
    const int16_t* c = scores + 4 * j;
    const long long cmin = std::min(std::min(c[0], c[1]), std::min(c[2], c[3])), cmax = std::max(std::max(c[0], c[1]), std::max(c[2], c[3]));
    next.assign((size_t)(hi + cmax - lo - cmin + 1), (u128_t)0);
    for (size_t k = 0; k < dist.size(); k++)
      if (dist[k])
        for (int b = 0; b < 4; b++) next[k + (size_t)(c[b] - cmin)] += dist[k];
    dist.swap(next);
    lo += cmin;
    hi += cmax;
  }
  // from the greatest score down: n_ge(s) = the sum from s on
  u128_t nge = 0, at = 0;
  long long t = hi + 1;
  for (long long s = hi; s >= lo; s--) {
    nge += dist[(size_t)(s - lo)];
    if (nge > K) break;
    t = s;
    at = nge;
  }
  if (threshold) *threshold = (int32_t)t;
  if (smin) *smin = (int32_t)lo;
  if (smax) *smax = (int32_t)hi;
  if (unreachable) *unreachable = t > hi ? 1 : 0;
  if (p_achieved) *p_achieved = std::ldexp((double)at, -2 * width);   // (one rounding of the count; the division is exact)
  return GX_OK;
}

static void put_motif_p(FILE* out, double p) {
  if (std::isnan(p)) fprintf(out, "\tNA");
  else fprintf(out, "\t%.3e", p);
}

// --motif-hits: one BED-like row per hit, in the order given
int gx_format_motif_hits(FILE* out, const char* const* names, const gx_region* peaks, const uint32_t* summit_off, size_t n_peaks,
                         const gx_motif* motifs, const char* const* ids, const char* const* motif_names, const double* p_threshold, int n_motifs,
                         const gx_motif_hit* hits, size_t n_hits) {
  if (!out || n_motifs < 0 || (n_hits && (!hits || !peaks || !summit_off || !names || !motifs || !ids || !motif_names || !p_threshold))) return GX_ERR_ORDER;
  for (size_t i = 0; i < n_hits; i++) {
    const gx_motif_hit& h = hits[i];
    if (h.region >= n_peaks || h.motif >= n_motifs || h.strand > 1) return GX_ERR_ORDER;
    if ((uint64_t)h.pos + motifs[h.motif].width > (uint64_t)peaks[h.region].end - peaks[h.region].start) return GX_ERR_ORDER;
  }
  fprintf(out, "chr\tstart\tend\tmotif\tscore\tstrand\tname\tpeak\toffset_from_summit\tp_threshold\n");
  for (size_t i = 0; i < n_hits; i++) {
    const gx_motif_hit& h = hits[i];
    const gx_region& k = peaks[h.region];
    const long L = (long)motifs[h.motif].width, at = (long)k.start + (long)h.pos;
    fprintf(out, "%s\t%ld\t%ld\t%s\t%.4f\t%c\t%s\tpeak_%u\t%ld", names[k.chrom], at, at + L, ids[h.motif], (double)h.score / 128.0, h.strand ? '-' : '+',
            motif_names[h.motif], h.region, (2 * at + L) / 2 - ((long)k.start + (long)summit_off[h.region]));
    put_motif_p(out, p_threshold[h.motif]);
    fprintf(out, "\n");
  }
  return GX_OK;
}

// --motif-summary: one row per motif
int gx_format_motif_summary(FILE* out, const gx_region* peaks, size_t n_peaks, const gx_motif* motifs, const char* const* ids,
                            const char* const* motif_names, const double* p_threshold, int n_motifs, const gx_motif_hit* hits, size_t n_hits,
                            const uint64_t* counts_peaks, const uint64_t* counts_genome) {
  if (!out || n_motifs < 0 || (n_peaks && !peaks) || (n_hits && !hits) ||
      (n_motifs && (!motifs || !ids || !motif_names || !p_threshold || !counts_peaks || !counts_genome)))
    return GX_ERR_ORDER;
  const size_t nM = (size_t)n_motifs;
  // the peaks with any hit of a motif: the hits come sorted by region, so a motif's last region tells a new one
  std::vector<uint64_t> withHit(nM, 0);
  std::vector<uint64_t> last(nM, ~0ull);
  for (size_t i = 0; i < n_hits; i++) {
    const gx_motif_hit& h = hits[i];
    if (h.region >= n_peaks || h.motif >= nM || (i && hits[i - 1].region > h.region)) return GX_ERR_ORDER;
    if (last[h.motif] != h.region) {
      last[h.motif] = h.region;
      withHit[h.motif]++;
    }
  }
  fprintf(out, "motif\tname\twidth\tthreshold\tp_threshold\tpeaks_scanned\tpeaks_with_hit\twindows_peaks\thits_peaks\twindows_genome\thits_genome\tenrichment\n");
  for (size_t m = 0; m < nM; m++) {
    uint64_t scanned = 0;
    for (size_t k = 0; k < n_peaks; k++)
      if (peaks[k].end > peaks[k].start && peaks[k].end - peaks[k].start >= motifs[m].width) scanned++;
    const u128_t hp = (u128_t)counts_peaks[nM + m] + counts_peaks[2 * nM + m], hg = (u128_t)counts_genome[nM + m] + counts_genome[2 * nM + m];
    const uint64_t wp = counts_peaks[m], wg = counts_genome[m];
    fprintf(out, "%s\t%s\t%u\t%.4f", ids[m], motif_names[m], motifs[m].width, (double)motifs[m].threshold / 128.0);
    put_motif_p(out, p_threshold[m]);
    fprintf(out, "\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu", (unsigned long long)scanned, (unsigned long long)withHit[m], (unsigned long long)wp,
            (unsigned long long)(uint64_t)hp, (unsigned long long)wg, (unsigned long long)(uint64_t)hg);
    if (hg == 0 || wp == 0) fprintf(out, "\tNA");
    else fprintf(out, "\t%.6f", to_double(mul128(hp, wg)) / to_double(mul128(hg, wp)));
    fprintf(out, "\n");
  }
  return GX_OK;
}

// --kmers (no Genrich counterpart): the strand collapse, the figures per canonical k-mer and the table.  Host only.
uint32_t gx_kmer_revcomp(int k, uint32_t code) {
  if (k < 1 || k > GX_KMER_MAX_K || (uint64_t)code >> (2 * k)) return 0xffffffffu;
  uint32_t r = 0;
  for (int j = 0; j < k; j++) {   // (the complement of digit b is 3 - b; the last base comes first)
    r = (r << 2) | (3u - (code & 3u));
    code >>= 2;
  }
  return r;
}

int gx_kmer_stats(int k, const uint64_t* counts_peaks, uint64_t windows_peaks, const uint64_t* counts_genome, uint64_t windows_genome,
                  gx_kmer_row* rows, size_t cap, size_t* n_rows) {
  if (k < 1 || k > GX_KMER_MAX_K || !counts_peaks || !counts_genome || (cap && !rows)) return GX_ERR_ORDER;
  const uint32_t nT = 1u << (2 * k);
  const uint64_t Wp = windows_peaks, Wg = windows_genome;
  std::vector<gx_kmer_row> all;
  for (uint32_t c = 0; c < nT; c++) {
    const uint32_t rc = gx_kmer_revcomp(k, c);
    if (rc < c) continue;   // (its canonical k-mer is rc)
    const u128_t cp128 = (u128_t)counts_peaks[c] + (rc != c ? counts_peaks[rc] : 0), cg128 = (u128_t)counts_genome[c] + (rc != c ? counts_genome[rc] : 0);
    if (cp128 > Wp || cg128 > Wg) return GX_ERR_ORDER;
    const uint64_t cp = (uint64_t)cp128, cg = (uint64_t)cg128;
    if (!cp) continue;
    gx_kmer_row r{c, rc, cp, cg, std::nan(""), std::nan("")};
    if (cg) {
      r.enrichment = to_double(mul128(cp, Wg)) / to_double(mul128(cg, Wp));
      if (cg != Wg)
        r.z = diff256(mul128(cp, Wg), mul128(cg, Wp), nullptr) / std::sqrt(to_double(mul128((u128_t)Wp * cg, (u128_t)(Wg - cg))));
    }
    all.push_back(r);
  }
  std::sort(all.begin(), all.end(), [](const gx_kmer_row& a, const gx_kmer_row& b) {
    const bool na = std::isnan(a.z), nb = std::isnan(b.z);
    if (na != nb) return nb;
    if (!na && a.z != b.z) return a.z > b.z;
    if (a.count_peaks != b.count_peaks) return a.count_peaks > b.count_peaks;
    return a.code < b.code;
  });
  if (n_rows) *n_rows = all.size();
  if (const size_t n = std::min(cap, all.size())) std::copy(all.begin(), all.begin() + n, rows);
  return GX_OK;
}

static void put_kmer(FILE* out, int k, uint32_t code) {
  char s[GX_KMER_MAX_K + 1];
  for (int j = 0; j < k; j++) s[j] = "ACGT"[(code >> (2 * (k - 1 - j))) & 3u];
  s[k] = '\0';
  fputs(s, out);
}

int gx_format_kmers(FILE* out, int k, int flank, uint64_t regions_counted, uint64_t windows_peaks, uint64_t windows_genome,
                    const uint64_t* counts_peaks, const uint64_t* counts_genome, int top) {
  if (!out || top < 0) return GX_ERR_ORDER;
  size_t n = 0;
  if (int rc = gx_kmer_stats(k, counts_peaks, windows_peaks, counts_genome, windows_genome, nullptr, 0, &n)) return rc;
  std::vector<gx_kmer_row> rows(std::max<size_t>(n, 1));
  if (int rc = gx_kmer_stats(k, counts_peaks, windows_peaks, counts_genome, windows_genome, rows.data(), n, nullptr)) return rc;
  fprintf(out, "# k=%d flank=", k);
  if (flank < 0) fprintf(out, "whole");
  else fprintf(out, "%d", flank);
  fprintf(out, " regions=%llu windows_peaks=%llu windows_genome=%llu kmers=%zu\n", (unsigned long long)regions_counted, (unsigned long long)windows_peaks,
          (unsigned long long)windows_genome, n);
  fprintf(out, "kmer\trevcomp\tcount_peaks\tcount_genome\tenrichment\tz\n");
  const size_t shown = top ? std::min<size_t>(n, (size_t)top) : n;
  for (size_t i = 0; i < shown; i++) {
    const gx_kmer_row& r = rows[i];
    put_kmer(out, k, r.code);
    fputc('\t', out);
    put_kmer(out, k, r.revcomp);
    fprintf(out, "\t%llu\t%llu", (unsigned long long)r.count_peaks, (unsigned long long)r.count_genome);
    if (std::isnan(r.enrichment)) fprintf(out, "\tNA");
    else fprintf(out, "\t%.6f", r.enrichment);
    if (std::isnan(r.z)) fprintf(out, "\tNA\n");
    else fprintf(out, "\t%.4f\n", r.z);
  }
  return GX_OK;
}

}  // extern "C"
