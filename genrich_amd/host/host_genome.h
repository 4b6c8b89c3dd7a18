// host_genome.h -- the FASTA reader behind --genome: a memory-mapped (or streamed) file to plain bases in 64-aligned staging
// buffers, sequence by sequence.  It knows nothing of the device or the run: a sink takes what it finds.
//
//   bool begin(const std::string& name)                       a '>' line: the name up to the first white space; false: skip it
//   bool bases(uint64_t first, const char* p, size_t n)       n stripped bases from base `first` on; `first` is a multiple of the
//                                                             chunk size (itself a multiple of 64); only a sequence's last
//                                                             call may have n below the chunk size.  false: stop (an error)
//   bool end(uint64_t length)                                 the sequence is complete.  false: stop (an error)
//
// Accepted: any line width, CRLF, empty lines, lower case, a last line without a newline, an empty sequence.  Stripped: every
// byte at or below the space character (newlines, carriage returns, blanks, tabs).  Everything else is a base to the sink, which
// classes it (N and the IUPAC codes are bases that are unknown).
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

namespace gxhost {

template <class Sink>
class FastaParser {
 public:
  // chunk: the staging buffer's bases, a multiple of 64
  FastaParser(Sink& sink, size_t chunk) : sink_(sink), chunk_(chunk), buf_(static_cast<char*>(aligned_alloc(64, chunk))) {}
  FastaParser(const FastaParser&) = delete;
  FastaParser& operator=(const FastaParser&) = delete;
  ~FastaParser() { free(buf_); }

  const std::string& error() const { return err_; }

  // the next n bytes of the file; false: an error (error()) or the sink said stop
  bool feed(const char* p, size_t n) {
    if (!buf_) return fail("cannot allocate the staging buffer");
    const char* const e = p + n;
    while (p < e) {
      if (lineStart_ && *p == '>') {
        if (!closeSeq()) return false;
        inHeader_ = true;
        nameDone_ = false;
        name_.clear();
        lineStart_ = false;
        p++;
        continue;
      }
      const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(e - p)));
      const char* stop = nl ? nl : e;
      if (inHeader_) {
        for (; p < stop && !nameDone_; p++) {
          if ((unsigned char)*p <= ' ') nameDone_ = true;
          else name_.push_back(*p);
        }
        p = stop;
        if (nl) {
          inHeader_ = false;
          inSeq_ = true;
          first_ = 0;
          fill_ = 0;
          skip_ = !sink_.begin(name_);
        }
      } else if (!inSeq_) {
        for (; p < stop; p++)
          if ((unsigned char)*p > ' ') return fail("not a FASTA file: text before the first '>' line");
      } else if (skip_) {
        p = stop;
      } else {
        while (p < stop) {
          // (the bytes of this line that fit the buffer, the white space dropped)
          size_t room = chunk_ - fill_;
          char* d = buf_ + fill_;
          while (p < stop && room) {
            const char c = *p++;
            if ((unsigned char)c > ' ') {
              *d++ = c;
              room--;
            }
          }
          fill_ = chunk_ - room;
          if (!room && !flush()) return false;
        }
      }
      if (nl) {
        p = nl + 1;
        lineStart_ = true;
      } else {
        lineStart_ = false;
      }
    }
    return true;
  }

  // the end of the file
  bool finish() {
    if (inHeader_) {   // a '>' line without a newline: an empty sequence
      inHeader_ = false;
      inSeq_ = true;
      first_ = 0;
      fill_ = 0;
      skip_ = !sink_.begin(name_);
    }
    return closeSeq();
  }

 private:
  bool fail(const char* what) {
    err_ = what;
    return false;
  }
  bool flush() {
    if (!sink_.bases(first_, buf_, fill_)) return false;
    first_ += fill_;
    fill_ = 0;
    return true;
  }
  bool closeSeq() {
    if (!inSeq_) return true;
    inSeq_ = false;
    if (skip_) return true;
    if (fill_ && !flush()) return false;
    return sink_.end(first_);
  }

  Sink& sink_;
  size_t chunk_;
  char* buf_;
  std::string name_, err_;
  bool lineStart_ = true, inHeader_ = false, nameDone_ = false, inSeq_ = false, skip_ = false;
  uint64_t first_ = 0;
  size_t fill_ = 0;
};

// A plain-text FASTA file through a mapping.  false: *err says why (the file cannot be read, it is gzip-compressed, it is no
// FASTA, or the sink's own sentence when it stopped and set *err).
template <class Sink>
bool genome_read_plain(const char* path, size_t chunk, Sink& sink, std::string* err) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) {
    *err = std::string("cannot read ") + path;
    return false;
  }
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
    close(fd);
    *err = std::string(path) + " is not a regular file (--genome maps its input)";
    return false;
  }
  const size_t len = (size_t)st.st_size;
  void* map = len ? mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
  close(fd);
  if (len && map == MAP_FAILED) {
    *err = std::string("cannot map ") + path;
    return false;
  }
  const char* p = static_cast<const char*>(map);
  bool ok = true;
  if (len >= 2 && (unsigned char)p[0] == 0x1f && (unsigned char)p[1] == 0x8b) {
    *err = std::string(path) + " is gzip-compressed";
    ok = false;
  } else {
    if (len) (void)madvise(map, len, MADV_SEQUENTIAL);
    FastaParser<Sink> fp(sink, chunk);
    const size_t step = (size_t)1 << 24;
    for (size_t at = 0; ok && at < len; at += step) ok = fp.feed(p + at, len - at < step ? len - at : step);
    ok = ok && fp.finish();
    if (!ok && err->empty()) *err = fp.error().empty() ? std::string("reading ") + path + " was stopped" : std::string(path) + ": " + fp.error();
  }
  if (len) munmap(map, len);
  return ok;
}

// ... through any reader with size_t read(void*, size_t) (bgzf_reader.h's Input: gzip and BGZF members inflated on the way)
template <class Reader, class Sink>
bool genome_read_stream(Reader& in, const char* path, size_t chunk, Sink& sink, std::string* err) {
  FastaParser<Sink> fp(sink, chunk);
  std::string block((size_t)1 << 22, '\0');
  bool ok = true;
  for (;;) {
    const size_t k = in.read(&block[0], block.size());
    if (!k) break;
    if (!(ok = fp.feed(block.data(), k))) break;
  }
  ok = ok && fp.finish();
  if (!ok && err->empty()) *err = fp.error().empty() ? std::string("reading ") + path + " was stopped" : std::string(path) + ": " + fp.error();
  return ok;
}

}  // namespace gxhost
