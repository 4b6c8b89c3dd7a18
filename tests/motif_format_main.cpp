// Stand-alone driver of gx_motif_pssm / gx_motif_threshold / gx_format_motif_hits / gx_format_motif_summary
// (genrich_amd/csrc/gx_emit.cpp) for tests/test_motifs.py, which compiles it together with gx_emit.cpp under
// -fsanitize=address,undefined and compares its output with tests/motifs_ref.py.  No device and no library: the C ABI entries
// gx_emit.cpp's other writers call are defined here and never reached.
//
// Spec file (argv[1]), per case:
//   "pssm L PC P", then four lines of L counts (rows A C G T).  Output: "refused <sentence>", or "scores" and the 4 L scores
//   (row j: A C G T), then "threshold t smin smax p unreachable" (p as %.17g).
//   "tables NP NM NH", then NP lines "chrom start end summit_off" (the names are chr0 .. chr9), NM lines "id name width threshold p"
//   (p may be nan), NH lines "region pos score motif strand", three lines of NM counts of the peaks and three of the genome.
//   Output: the hits table, "--", the summary table.
// Every case's output ends with "--\n".
#include <cinttypes>
#include <cmath>
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

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  const char* names[10] = {"chr0", "chr1", "chr2", "chr3", "chr4", "chr5", "chr6", "chr7", "chr8", "chr9"};
  char kind[16];
  while (fscanf(f, "%15s", kind) == 1) {
    if (!strcmp(kind, "pssm")) {
      int L = 0;
      double pc = 0, p = 0;
      if (fscanf(f, "%d %lf %lf", &L, &pc, &p) != 3 || L < 0 || L > 64) return 2;
      // (exact-size heap arrays: a read or a write beyond them is the sanitizer's to catch)
      std::vector<uint32_t> counts((size_t)4 * (size_t)L);
      for (uint32_t& v : counts)
        if (fscanf(f, "%" SCNu32, &v) != 1) return 2;
      std::vector<int16_t> scores((size_t)4 * (size_t)(L > 32 ? 0 : L));
      int32_t lo = 0, hi = 0;
      std::vector<char> why(96);
      if (gx_motif_pssm(counts.data(), L, pc, scores.data(), &lo, &hi, why.data(), why.size()) != GX_OK) {
        printf("refused %s\n--\n", why.data());
        continue;
      }
      printf("scores");
      for (int16_t s : scores) printf(" %d", (int)s);
      int32_t t = 0, lo2 = 0, hi2 = 0;
      double pa = 0;
      int un = 0;
      if (gx_motif_threshold(scores.data(), L, p, &t, &lo2, &hi2, &pa, &un) != GX_OK || lo2 != lo || hi2 != hi) return 5;
      printf("\nthreshold %d %d %d %.17g %d\n", t, lo, hi, pa, un);
    } else if (!strcmp(kind, "tables")) {
      size_t NP = 0, NM = 0, NH = 0;
      if (fscanf(f, "%zu %zu %zu", &NP, &NM, &NH) != 3) return 2;
      std::vector<gx_region> reg(NP);
      std::vector<uint32_t> summit(NP);
      for (size_t i = 0; i < NP; i++)
        if (fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &reg[i].chrom, &reg[i].start, &reg[i].end, &summit[i]) != 4 || reg[i].chrom > 9) return 2;
      std::vector<gx_motif> mot(NM);
      std::vector<std::string> ids(NM), mn(NM);
      std::vector<double> pthr(NM);
      for (size_t i = 0; i < NM; i++) {
        char a[64], b[64];
        if (fscanf(f, "%63s %63s %" SCNu32 " %" SCNd32 " %lf", a, b, &mot[i].width, &mot[i].threshold, &pthr[i]) != 5) return 2;
        mot[i].offset = 0;
        ids[i] = a;
        mn[i] = b;
      }
      std::vector<const char*> pid, pmn;
      for (size_t i = 0; i < NM; i++) {
        pid.push_back(ids[i].c_str());
        pmn.push_back(mn[i].c_str());
      }
      std::vector<gx_motif_hit> hits(NH);
      for (size_t i = 0; i < NH; i++) {
        unsigned m = 0, s = 0;
        if (fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNd32 " %u %u", &hits[i].region, &hits[i].pos, &hits[i].score, &m, &s) != 5) return 2;
        hits[i].motif = (uint16_t)m;
        hits[i].strand = (uint8_t)s;
        hits[i].pad = 0;
      }
      std::vector<uint64_t> cp(3 * NM), cg(3 * NM);
      for (uint64_t& v : cp)
        if (fscanf(f, "%" SCNu64, &v) != 1) return 2;
      for (uint64_t& v : cg)
        if (fscanf(f, "%" SCNu64, &v) != 1) return 2;
      if (int rc = gx_format_motif_hits(stdout, names, reg.data(), summit.data(), NP, mot.data(), pid.data(), pmn.data(), pthr.data(), (int)NM, hits.data(), NH))
        return 10 - rc;
      printf("--\n");
      if (int rc = gx_format_motif_summary(stdout, reg.data(), NP, mot.data(), pid.data(), pmn.data(), pthr.data(), (int)NM, hits.data(), NH, cp.data(), cg.data()))
        return 10 - rc;
    } else {
      return 2;
    }
    printf("--\n");
  }
  fclose(f);
  // the argument checks: nothing written, GX_ERR_ORDER
  const uint32_t c4[4] = {1, 2, 3, 4};
  int16_t s4[4];
  if (gx_motif_pssm(nullptr, 1, 1.0, s4, nullptr, nullptr, nullptr, 0) != GX_ERR_ORDER || gx_motif_pssm(c4, 1, 1.0, nullptr, nullptr, nullptr, nullptr, 0) != GX_ERR_ORDER ||
      gx_motif_pssm(c4, 0, 1.0, s4, nullptr, nullptr, nullptr, 0) != GX_ERR_ORDER || gx_motif_pssm(c4, 1, -1.0, s4, nullptr, nullptr, nullptr, 0) != GX_ERR_ORDER)
    return 3;
  if (gx_motif_pssm(c4, 1, 1.0, s4, nullptr, nullptr, nullptr, 0) != GX_OK) return 3;
  int32_t t = 0;
  if (gx_motif_threshold(s4, 1, 0.0, &t, nullptr, nullptr, nullptr, nullptr) != GX_ERR_ORDER || gx_motif_threshold(s4, 1, 1.5, &t, nullptr, nullptr, nullptr, nullptr) != GX_ERR_ORDER ||
      gx_motif_threshold(s4, 33, 0.5, &t, nullptr, nullptr, nullptr, nullptr) != GX_ERR_ORDER || gx_motif_threshold(nullptr, 1, 0.5, &t, nullptr, nullptr, nullptr, nullptr) != GX_ERR_ORDER)
    return 3;
  if (gx_motif_threshold(s4, 1, 0.5, &t, nullptr, nullptr, nullptr, nullptr) != GX_OK) return 3;
  const gx_region one = {0, 10, 20};
  const uint32_t so = 3;
  const gx_motif m1 = {6, 0, 0};
  const char* id = "M";
  const double p1 = 0.5;
  const gx_motif_hit far = {0, 5, 0, 0, 0, 0}, other = {1, 0, 0, 0, 0, 0}, nomotif = {0, 0, 0, 1, 0, 0};
  if (gx_format_motif_hits(stdout, names, &one, &so, 1, &m1, &id, &id, &p1, 1, &far, 1) != GX_ERR_ORDER ||      // the window leaves the peak
      gx_format_motif_hits(stdout, names, &one, &so, 1, &m1, &id, &id, &p1, 1, &other, 1) != GX_ERR_ORDER ||    // a peak the list does not have
      gx_format_motif_hits(stdout, names, &one, &so, 1, &m1, &id, &id, &p1, 1, &nomotif, 1) != GX_ERR_ORDER || gx_format_motif_hits(nullptr, names, &one, &so, 1, &m1, &id, &id, &p1, 1, &far, 0) != GX_ERR_ORDER)
    return 3;
  const uint64_t c3[3] = {1, 1, 1};
  if (gx_format_motif_summary(stdout, &one, 1, &m1, &id, &id, &p1, 1, &other, 1, c3, c3) != GX_ERR_ORDER || gx_format_motif_summary(stdout, &one, 1, &m1, &id, &id, &p1, 1, nullptr, 0, nullptr, c3) != GX_ERR_ORDER)
    return 3;
  return 0;
}
