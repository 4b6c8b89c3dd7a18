// host_common.h -- what every part of the host program uses: die(), the number parsers, output files (plain or gzip) and the input
// stream.  (a part of genrich_amd.cpp's translation unit, like the headers below: they are included in this order)
#pragma once
namespace {

// A decoding thread (parallel record decoding, below) must not end the program: an earlier record, still on its way
// through the run's state, may have a warning to print or an error of its own.  With t_capture set, die() keeps the
// message and unwinds to the decoder; the thread that owns the state dies with it when that record's turn comes.
struct DecodeAbort {};
thread_local std::pair<std::string, std::string>* t_capture = nullptr;

[[noreturn]] void die(const std::string& msg, const char* tail) {  // error(), Genrich.c:78-81
  if (t_capture) {
    *t_capture = {msg, tail};
    throw DecodeAbort{};
  }
  fprintf(stderr, "Error! %s%s\n", msg.c_str(), tail);
  // What the reference's exit() does that can be seen from outside is flushing its open streams; the reader, decoder,
  // inflate and state threads of the ingest may still be running here, so nothing else is torn down under them (no
  // static destructors, no atexit handlers -- the HIP runtime's among them -- next to live threads).
  fflush(nullptr);
  _exit(EXIT_FAILURE);
}

int getInt(const char* s) {  // 102-108
  char* end;
  long v = strtol(s, &end, 10);
  if (*end != '\0') die(s, ": cannot convert to int");
  return (int)v;
}
long getLong(const char* s) {
  char* end;
  long v = strtol(s, &end, 10);
  if (*end != '\0') die(s, ": cannot convert to int");
  return v;
}
float getFloat(const char* s) {  // 90-96
  char* end;
  float v = strtof(s, &end);
  if (*end != '\0') die(s, ": cannot convert to float");
  return v;
}
// a list option (-t a,b,c) cut at its commas and blanks; no option, no items
std::vector<std::string> splitList(const char* list) {
  std::vector<std::string> out;
  std::string l(list ? list : "");
  for (char* t = strtok(l.data(), ", "); t; t = strtok(nullptr, ", ")) out.push_back(t);
  return out;
}
// The long options' own numbers: a decimal integer in [lo, hi] and nothing else -- no blank, a sign only where the range reaches
// below zero, nothing behind the digits.  With `rest` the number may be an item of a list: a comma may follow, and *rest is what
// stands behind it (nullptr behind the last item).  false for everything else; the sentence is the caller's.
bool strictInt(const char* s, __int128 lo, __int128 hi, __int128* v, const char** rest = nullptr) {
  const bool neg = lo < 0 && *s == '-';
  if (lo < 0 && (*s == '-' || *s == '+')) s++;
  if (!isdigit((unsigned char)*s)) return false;
  char* end;
  errno = 0;
  const unsigned long long mag = strtoull(s, &end, 10);
  if (errno == ERANGE || (*end != '\0' && !(rest && *end == ','))) return false;
  *v = neg ? -(__int128)mag : (__int128)mag;
  if (rest) *rest = *end ? end + 1 : nullptr;
  return *v >= lo && *v <= hi;
}

// ---- output files: plain or gzip (-z), printf-style ---------------------------------------
struct Out {
  FILE* f = nullptr;
  gzFile gz = nullptr;
  std::string name;
};

ssize_t gzCookieWrite(void* c, const char* buf, size_t n) { return gzwrite((gzFile)c, buf, (unsigned)n) ? (ssize_t)n : 0; }
int gzCookieClose(void* c) { return gzclose((gzFile)c) == Z_OK ? 0 : -1; }

Out openWrite(const char* path, bool gzOut) {  // openWrite, 5076-5102
  Out o;
  if (path[0] == '-' && strlen(path) > 1) die(path, ": output filename cannot start with '-'");
  bool isStdout = !strcmp(path, "-");
  o.name = path;
  if (gzOut) {
    if (!isStdout && (o.name.size() < 3 || o.name.compare(o.name.size() - 3, 3, ".gz"))) o.name += ".gz";
    gzFile g = isStdout ? gzdopen(fileno(stdout), "wb") : gzopen(o.name.c_str(), "w");
    if (!g) die(o.name, ": cannot open file for writing");
    cookie_io_functions_t io = {nullptr, gzCookieWrite, nullptr, gzCookieClose};
    o.f = fopencookie(g, "w", io);
    o.gz = g;
  } else
    o.f = isStdout ? stdout : fopen(path, "w");
  if (!o.f) die(o.name, ": cannot open file for writing");
  return o;
}
void closeOut(Out& o) {
  if (o.f && o.f != stdout && fclose(o.f)) die(o.name, ": cannot close file");
  if (o.f == stdout) fflush(stdout);
  o.f = nullptr;
}

// ---- input: one gz-transparent byte stream (plain, gzip or BGZF) ------------------------------
// (BGZF members are inflated by a pool of threads, bgzf_reader.h; everything else through zlib's gz*)
typedef gxhost::Input In;
void openRead(In& in, const char* path, int inflaters) {
  if (!in.open(path, inflaters)) die(path, ": cannot open file for reading");
}
void checkIn(In& in) {
  if (!in.error().empty()) die(in.name(), (": " + in.error()).c_str());
}

}  // namespace
