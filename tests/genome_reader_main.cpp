// Stand-alone driver of the FASTA reader (genrich_amd/host/host_genome.h) for tests/test_gcbias.py, which compiles it under
// -fsanitize=address,undefined.  No device and no library.
//
// argv: FASTA CHUNK [SKIP_NAME].  Output (stdout): per sequence that is not skipped one line
// "name length gc acgt checksum" -- gc / acgt as the device classes a byte (G C g c; A C G T a c g t), the checksum FNV-1a (64 bits)
// over the stripped bases.  The sink checks the reader's promises: every call starts on a multiple of CHUNK, only a sequence's
// last call is shorter, the bases hold no white space, the length is the bases' sum.  Exit 0; 3: a promise broken; 1: the
// reader's error, its sentence on stderr.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../genrich_amd/host/host_genome.h"

struct Sink {
  size_t chunk;
  std::string skip;
  std::string name;
  uint64_t got = 0, gc = 0, acgt = 0, sum = 0;
  bool shortSeen = false, broken = false;
  bool begin(const std::string& n) {
    if (!skip.empty() && n == skip) return false;
    name = n;
    got = gc = acgt = 0;
    sum = 1469598103934665603ull;
    shortSeen = false;
    return true;
  }
  bool bases(uint64_t first, const char* p, size_t n) {
    if (first != got || first % chunk || shortSeen || !n || n > chunk || ((uintptr_t)p & 63)) broken = true;
    if (n < chunk) shortSeen = true;
    for (size_t i = 0; i < n; i++) {
      const unsigned char c = (unsigned char)p[i];
      if (c <= ' ') broken = true;
      const unsigned char l = c | 0x20;
      const bool g = l == 'g' || l == 'c';
      gc += g;
      acgt += g || l == 'a' || l == 't';
      sum = (sum ^ c) * 1099511628211ull;
    }
    got += n;
    return !broken;
  }
  bool end(uint64_t length) {
    if (length != got) broken = true;
    printf("%s %" PRIu64 " %" PRIu64 " %" PRIu64 " %016" PRIx64 "\n", name.c_str(), length, gc, acgt, sum);
    return !broken;
  }
};

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  Sink s;
  s.chunk = (size_t)strtoull(argv[2], nullptr, 10);
  if (!s.chunk || s.chunk % 64) return 2;
  if (argc > 3) s.skip = argv[3];
  std::string err;
  const bool ok = gxhost::genome_read_plain(argv[1], s.chunk, s, &err);
  if (s.broken) return 3;
  if (!ok) {
    fprintf(stderr, "%s\n", err.c_str());
    return 1;
  }
  return 0;
}
