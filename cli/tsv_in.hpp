// tsv_in.hpp — what the host-only commands that READ search results (kmcp-filter, kmcp-regions) share: whole lines of a plain or gzip
// file, and the reference's strconv.ParseFloat of one field.
#pragma once
#include <zlib.h>

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tsv_out.hpp"

namespace tsv_in {

using tsv_out::die;

// gz-or-plain reader of whole lines, end-of-line kept (zlib reads plain files transparently)
struct RawLines {
  gzFile f = nullptr;
  std::vector<char> buf;
  size_t pos = 0, end = 0;
  bool eof = false;
  explicit RawLines(const std::string& path) : buf(1 << 20) {
    f = path == "-" ? gzdopen(0, "rb") : gzopen(path.c_str(), "rb");
    if (!f) die("%s: %s", path.c_str(), strerror(errno));
    gzbuffer(f, 1 << 18);
  }
  ~RawLines() {
    if (f) gzclose(f);
  }
  bool fill() {
    if (eof) return false;
    if (pos > 0) {
      memmove(buf.data(), buf.data() + pos, end - pos);
      end -= pos;
      pos = 0;
    }
    if (end == buf.size()) buf.resize(buf.size() * 2);
    const int n = gzread(f, buf.data() + end, (unsigned)(buf.size() - end));
    if (n < 0) die("read error");
    if (n == 0) {
      eof = true;
      return false;
    }
    end += (size_t)n;
    return true;
  }
  // the next line inside the buffer (valid until the next call); *n includes its '\n' when it has one
  bool next(const char** p, size_t* n) {
    for (;;) {
      const char* nl = (const char*)memchr(buf.data() + pos, '\n', end - pos);
      if (nl) {
        *p = buf.data() + pos;
        *n = (size_t)(nl - *p) + 1;
        pos += *n;
        return true;
      }
      if (!fill()) {
        if (pos == end) return false;
        *p = buf.data() + pos;
        *n = end - pos;
        pos = end;
        return true;
      }
    }
  }
};

// strconv.ParseFloat of a field: the whole field must be a number
inline bool parse_float(const char* p, size_t n, double* v) {
  if (n == 0 || n > 63 || p[0] == ' ' || p[0] == '\t') return false;
  char tmp[64];
  memcpy(tmp, p, n);
  tmp[n] = 0;
  char* e = nullptr;
  *v = strtod(tmp, &e);
  return e == tmp + n;
}

// as much of filepath.Clean as two spellings of one path usually differ by
inline std::string clean_path(std::string p) {
  std::string o = !p.empty() && p[0] == '/' ? "/" : "";  // empty and "." components go, ".." stays
  for (size_t at = 0; at <= p.size();) {
    const size_t e = std::min(p.find('/', at), p.size());
    if (e > at && !(e - at == 1 && p[at] == '.')) {
      if (!o.empty() && o.back() != '/') o.push_back('/');
      o.append(p, at, e - at);
    }
    at = e + 1;
  }
  return o.empty() ? "." : o;
}

}  // namespace tsv_in
