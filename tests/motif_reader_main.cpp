// Stand-alone driver of the JASPAR reader (genrich_amd/host/host_motifs.h) for tests/test_motifs.py, which compiles it under
// -fsanitize=address,undefined.  No device and no library.
//
// argv: FILE [PIECE].  Without PIECE the file goes through the mapping (motifs_read_plain); with it, through the push parser in
// pieces of PIECE bytes.  Output (stdout): per motif one line "id<TAB>name<TAB>width<TAB>the 4 x width counts, rows A C G T".
// Exit 0; 1: the reader's error, its sentence on stderr.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../genrich_amd/host/host_motifs.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::vector<gxhost::MotifRec> motifs;
  std::string err;
  bool ok;
  if (argc > 2) {
    const size_t piece = (size_t)strtoull(argv[2], nullptr, 10);
    if (!piece) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<char> buf(piece);
    gxhost::JasparParser jp(motifs);
    ok = true;
    for (size_t k; ok && (k = fread(buf.data(), 1, piece, f)) > 0;) {
      std::vector<char> exact(buf.begin(), buf.begin() + (long)k);   // (an allocation of exactly the piece: a read past it is seen)
      ok = jp.feed(exact.data(), k);
    }
    fclose(f);
    ok = ok && jp.finish();
    err = jp.error();
  } else {
    ok = gxhost::motifs_read_plain(argv[1], motifs, &err);
  }
  if (!ok) {
    fprintf(stderr, "%s\n", err.c_str());
    return 1;
  }
  for (const gxhost::MotifRec& m : motifs) {
    printf("%s\t%s\t%u\t", m.id.c_str(), m.name.c_str(), m.width);
    for (size_t i = 0; i < m.counts.size(); i++) printf("%s%u", i ? " " : "", m.counts[i]);
    printf("\n");
  }
  return 0;
}
