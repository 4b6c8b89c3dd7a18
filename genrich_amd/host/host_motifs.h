// host_motifs.h -- the JASPAR reader behind --motifs: a memory-mapped file to count matrices, motif by motif.  It knows nothing
// of the device or the run.  Both forms of the format:
//
//   >ID NAME                      >ID NAME
//   A [ n n ... ]                 n n ...        (four bare rows in the order A C G T)
//   C [ n n ... ]                 n n ...
//   G [ n n ... ]                 n n ...
//   T [ n n ... ]                 n n ...
//
// Accepted: any white space, CRLF, blank lines, a last line without a newline, a header without a NAME (the ID stands in).
// Refused, with the motif's ID and a sentence: a width of 0 or above 32, rows of unequal length, a count that is no integer
// from 0 to 2^31 - 1, fewer or more than four rows, lettered rows out of the order A C G T, a repeated ID, more than 4096
// motifs, a row before the first header, a file without a motif.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

namespace gxhost {

constexpr size_t MOTIF_MAX_WIDTH = 32, MOTIF_MAX = 4096;

struct MotifRec {
  std::string id, name;
  uint32_t width = 0;
  std::vector<uint32_t> counts;   // [4][width], rows A C G T
};

class JasparParser {
 public:
  explicit JasparParser(std::vector<MotifRec>& out) : out_(out) {}
  const std::string& error() const { return err_; }

  // the next n bytes of the file; false: an error (error())
  bool feed(const char* p, size_t n) {
    const char* const e = p + n;
    while (p < e) {
      const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(e - p)));
      line_.append(p, nl ? nl : e);
      if (!nl) break;
      if (!takeLine()) return false;
      p = nl + 1;
    }
    return true;
  }
  // the end of the file
  bool finish() {
    if (!line_.empty() && !takeLine()) return false;
    if (!closeMotif()) return false;
    if (out_.empty()) return fail("", "no motif in the file");
    return true;
  }

 private:
  bool fail(const std::string& id, const char* what) {
    err_ = (id.empty() ? std::string() : id + ": ") + what;
    return false;
  }
  static bool blank(char c) { return (unsigned char)c <= ' '; }
  bool closeMotif() {
    if (!open_) return true;
    open_ = false;
    if (rows_.size() != 4) return fail(cur_.id, "fewer than four rows");
    for (const auto& r : rows_)
      if (r.size() != rows_[0].size()) return fail(cur_.id, "rows of unequal length");
    if (rows_[0].empty() || rows_[0].size() > MOTIF_MAX_WIDTH) return fail(cur_.id, "the width must be 1 to 32");
    cur_.width = (uint32_t)rows_[0].size();
    cur_.counts.clear();
    for (const auto& r : rows_) cur_.counts.insert(cur_.counts.end(), r.begin(), r.end());
    out_.push_back(cur_);
    return true;
  }
  bool takeLine() {
    std::string s;
    s.swap(line_);
    size_t a = 0, b = s.size();
    while (a < b && blank(s[a])) a++;
    while (b > a && blank(s[b - 1])) b--;
    if (a == b) return true;
    if (s[a] == '>') {
      if (!closeMotif()) return false;
      size_t i = a + 1;
      while (i < b && blank(s[i])) i++;
      size_t j = i;
      while (j < b && !blank(s[j])) j++;
      if (i == j) return fail("?", "a header without an ID");
      cur_ = MotifRec{};
      cur_.id = s.substr(i, j - i);
      while (j < b && blank(s[j])) j++;
      cur_.name = j < b ? s.substr(j, b - j) : cur_.id;
      if (!seen_.insert(cur_.id).second) return fail(cur_.id, "a repeated ID");
      if (seen_.size() > MOTIF_MAX) return fail(cur_.id, "more than 4096 motifs");
      rows_.clear();
      open_ = true;
      return true;
    }
    if (!open_) return fail("?", "a row before the first header");
    if (rows_.size() == 4) return fail(cur_.id, "more than four rows");
    const char first = (char)(s[a] & ~0x20);
    if (first == 'A' || first == 'C' || first == 'G' || first == 'T') {
      if (first != "ACGT"[rows_.size()]) return fail(cur_.id, "rows out of the order A C G T");
      a++;
    }
    std::vector<uint32_t> row;
    while (a < b) {
      if (blank(s[a]) || s[a] == '[' || s[a] == ']') {
        a++;
        continue;
      }
      uint64_t v = 0;
      size_t k = a;
      for (; k < b && !blank(s[k]) && s[k] != '[' && s[k] != ']'; k++) {
        if (s[k] < '0' || s[k] > '9' || v >> 31) return fail(cur_.id, "a count that is not an integer from 0 to 2^31 - 1");
        v = v * 10 + (uint64_t)(s[k] - '0');
      }
      if (v >> 31) return fail(cur_.id, "a count that is not an integer from 0 to 2^31 - 1");
      row.push_back((uint32_t)v);
      a = k;
    }
    rows_.push_back(std::move(row));
    return true;
  }

  std::vector<MotifRec>& out_;
  std::string line_, err_;
  MotifRec cur_;
  std::vector<std::vector<uint32_t>> rows_;
  std::unordered_set<std::string> seen_;
  bool open_ = false;
};

// A plain-text JASPAR file through a mapping.  false: *err says why
inline bool motifs_read_plain(const char* path, std::vector<MotifRec>& out, std::string* err) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) {
    *err = std::string("cannot read ") + path;
    return false;
  }
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
    close(fd);
    *err = std::string(path) + " is not a regular file (--motifs maps its input)";
    return false;
  }
  const size_t len = (size_t)st.st_size;
  void* map = len ? mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
  close(fd);
  if (len && map == MAP_FAILED) {
    *err = std::string("cannot map ") + path;
    return false;
  }
  JasparParser jp(out);
  const char* p = static_cast<const char*>(map);
  bool ok = true;
  const size_t step = (size_t)1 << 16;
  for (size_t at = 0; ok && at < len; at += step) ok = jp.feed(p + at, len - at < step ? len - at : step);
  ok = ok && jp.finish();
  if (!ok) *err = jp.error();
  if (len) munmap(map, len);
  return ok;
}

}  // namespace gxhost
