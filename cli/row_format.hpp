// row_format.hpp — kmcp-search's output side (header only): the out file (plain or multi-member .gz), the TSV row formatter and the pool of
// formatter threads.  The including program provides die().
#pragma once
#include <errno.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../include/kmcp_gpu.h"

[[noreturn]] void die(const char* fmt, ...);  // log the message and exit(255), like the reference's checkError

// one complete gzip member holding `in` (deflate level 6 as compress/gzip's default in the reference's outStream)
static inline std::string gzip_member(const std::string& in) {
  z_stream z;
  memset(&z, 0, sizeof z);
  if (deflateInit2(&z, 6, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) die("zlib: deflateInit2 failed");
  std::string out;
  out.resize(deflateBound(&z, (uLong)in.size()) + 64);
  z.next_in = (Bytef*)in.data();
  z.avail_in = (uInt)in.size();
  z.next_out = (Bytef*)&out[0];
  z.avail_out = (uInt)out.size();
  if (deflate(&z, Z_FINISH) != Z_STREAM_END) die("zlib: deflate failed");
  out.resize(z.total_out);
  deflateEnd(&z);
  return out;
}

class Out {
 public:
  explicit Out(const std::string& path) {
    gz_ = path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0;
    f_ = path == "-" ? stdout : fopen(path.c_str(), "wb");
    if (!f_) die("%s: %s", path.c_str(), strerror(errno));
  }
  bool gz() const { return gz_; }
  // text: compressed here when the file is .gz
  void write(const std::string& s) {
    if (s.empty()) return;
    if (gz_) write_raw(gzip_member(s));
    else write_raw(s);
  }
  // bytes that are already in the file's encoding
  void write_raw(const std::string& s) {
    if (!s.empty() && fwrite(s.data(), 1, s.size(), f_) != s.size()) die("write failed: %s", strerror(errno));
  }
  void close() {
    if (f_ != stdout) fclose(f_);
    else fflush(f_);
  }

 private:
  bool gz_ = false;
  FILE* f_ = nullptr;
};

// ---- TSV rows.  Number formatting must equal Go's strconv (FormatFloat 'f',4 / 'e',4 = correctly rounded decimals, which is
// what printf gives); the fast paths below produce the same digits and fall back to snprintf whenever a rounding tie is near.
struct RowFormatter {
  // text buffers this formatter has filled before (the flusher hands them back): the next part is written where this thread's last ones were
  std::mutex free_mu;
  std::vector<std::string> free_bufs;
  void take(std::string& into) {
    std::lock_guard<std::mutex> g(free_mu);
    if (free_bufs.empty()) return;
    into = std::move(free_bufs.back());
    free_bufs.pop_back();
    into.clear();
  }
  void give_back(std::string&& s) {
    if (s.capacity() > (1ull << 30)) return;
    std::lock_guard<std::mutex> g(free_mu);
    if (free_bufs.size() < 64) free_bufs.push_back(std::move(s));
  }
  char tmp[64];
  std::vector<kmcpg_match> scratch;  // the records of the query being formatted (kmcpg_expand_pairs)
  std::unordered_map<uint64_t, std::string> fpr_cache;  // the FPR of a match depends on (qKmers, mKmers) only

  // A row is assembled in a fixed scratch line through a moving pointer (no capacity checks per character) and appended to the
  // batch's text in one go; rows that could not fit (IDs or target names of kilobytes) take the std::string path below.
  static char* w_u64(char* p, uint64_t v) {
    char t[24];
    int n = 0;
    do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) *p++ = t[--n];
    return p;
  }
  static char* w_i(char* p, int64_t v) {
    if (v < 0) { *p++ = '-'; return w_u64(p, (uint64_t)(-v)); }
    return w_u64(p, (uint64_t)v);
  }
  static char* w_f4(char* p, double v) {  // "%.4f"
    if (v >= 0 && v < 1e5) {  // v * 10000 < 1e9: its rounding error (< 2e-7) cannot carry the fraction across the 1e-6 guard below
      const double sc = v * 10000.0;
      const double fl = floor(sc);
      const double fr = sc - fl;
      if (fabs(fr - 0.5) > 1e-6) {  // far from a tie: the scaled value rounds like the exact decimal expansion
        const uint64_t q = (uint64_t)fl + (fr > 0.5 ? 1 : 0);
        p = w_u64(p, q / 10000);
        *p++ = '.';
        const unsigned f = (unsigned)(q % 10000);
        *p++ = (char)('0' + f / 1000);
        *p++ = (char)('0' + f / 100 % 10);
        *p++ = (char)('0' + f / 10 % 10);
        *p++ = (char)('0' + f % 10);
        return p;
      }
    }
    return p + snprintf(p, 48, "%.4f", v);
  }
  static void put_u64(std::string& b, uint64_t v) {
    char t[24];
    b.append(t, (size_t)(w_u64(t, v) - t));
  }
  static void put_i(std::string& b, int64_t v) {
    char t[24];
    b.append(t, (size_t)(w_i(t, v) - t));
  }
  void put_f4(std::string& b, double v) {
    char t[64];
    b.append(t, (size_t)(w_f4(t, v) - t));
  }
  // FPR strings of short queries by (n, c) in a table, the rest in a map
  std::vector<std::vector<std::string>> fpr_tab;
  const std::string& fpr(int n, int c, double v) {
    if (n > 0 && n <= 4096 && c >= 0 && c <= n) {
      if (fpr_tab.empty()) fpr_tab.resize(4097);
      std::vector<std::string>& row_of_n = fpr_tab[(size_t)n];
      if (row_of_n.empty()) row_of_n.resize((size_t)n + 1);
      std::string& e = row_of_n[(size_t)c];
      if (e.empty()) e.assign(tmp, (size_t)snprintf(tmp, sizeof tmp, "%.4e", v));
      return e;
    }
    const uint64_t key = ((uint64_t)(uint32_t)n << 32) | (uint32_t)c;
    auto it = fpr_cache.find(key);
    if (it != fpr_cache.end()) return it->second;
    if (fpr_cache.size() > (1u << 20)) fpr_cache.clear();
    return fpr_cache.emplace(key, std::string(tmp, (size_t)snprintf(tmp, sizeof tmp, "%.4e", v))).first->second;
  }
  static constexpr size_t LINE = 8192;
  char line[LINE];
  void row(std::string& b, std::string_view id, int qlen, int qkmers, uint64_t hits, const std::string& target, const kmcpg_match& m, int k,
           uint64_t qidx) {
    const std::string& f = fpr(qkmers, m.mkmers, m.fpr);
    if (id.size() + target.size() + f.size() + 400 > LINE) {  // oversized names: the slow, unbounded path
      b += id; b.push_back('\t'); put_i(b, qlen); b.push_back('\t'); put_i(b, qkmers); b.push_back('\t');
      b += f; b.push_back('\t'); put_u64(b, hits); b.push_back('\t');
      b += target; b.push_back('\t'); put_u64(b, (uint16_t)m.target_idx); b.push_back('\t'); put_u64(b, m.target_idx >> 16); b.push_back('\t');
      put_u64(b, m.gsize); b.push_back('\t'); put_i(b, k); b.push_back('\t'); put_i(b, m.mkmers); b.push_back('\t');
      put_f4(b, m.qcov); b.push_back('\t'); put_f4(b, m.tcov); b.push_back('\t'); put_f4(b, m.jacc); b.push_back('\t');
      put_u64(b, qidx); b.push_back('\n');
      return;
    }
    char* p = line;
    memcpy(p, id.data(), id.size()); p += id.size(); *p++ = '\t';
    p = w_i(p, qlen); *p++ = '\t';
    p = w_i(p, qkmers); *p++ = '\t';
    memcpy(p, f.data(), f.size()); p += f.size(); *p++ = '\t';
    p = w_u64(p, hits); *p++ = '\t';
    memcpy(p, target.data(), target.size()); p += target.size(); *p++ = '\t';
    p = w_u64(p, (uint16_t)m.target_idx); *p++ = '\t';
    p = w_u64(p, m.target_idx >> 16); *p++ = '\t';
    p = w_u64(p, m.gsize); *p++ = '\t';
    p = w_i(p, k); *p++ = '\t';
    p = w_i(p, m.mkmers); *p++ = '\t';
    p = w_f4(p, m.qcov); *p++ = '\t';
    p = w_f4(p, m.tcov); *p++ = '\t';
    p = w_f4(p, m.jacc); *p++ = '\t';
    p = w_u64(p, qidx); *p++ = '\n';
    b.append(line, (size_t)(p - line));
  }
  // All rows of one query.  With many matches (a database full of close relatives: hundreds per read) what is the same in every
  // row — ID, qLen, qKmers in front, hits, kSize, queryIdx — is formatted once, and what depends on the column only (target,
  // chunkIdx, chunks, tLen) once per column and formatter thread; a row then costs one integer, three fixed-point numbers and
  // a few copies.
  std::vector<std::string> col_text;  // "target\tchunkIdx\tchunks\ttLen\t" by column, filled on first use
  void rows(std::string& b, std::string_view id, int qlen, int qkmers, const kmcpg_match* ms, uint64_t cnt, const std::vector<std::string>& target,
            int k, uint64_t qidx) {
    if (cnt < 4 || id.size() > 1024) {
      for (uint64_t j = 0; j < cnt; j++) row(b, id, qlen, qkmers, cnt, target[ms[j].col], ms[j], k, qidx);
      return;
    }
    char pre[1024 + 64], mid[32], ks[24], suf[32];
    char* q = pre;
    memcpy(q, id.data(), id.size()); q += id.size(); *q++ = '\t';
    q = w_i(q, qlen); *q++ = '\t';
    q = w_i(q, qkmers); *q++ = '\t';
    const size_t pre_n = (size_t)(q - pre);
    q = w_u64(mid, cnt); *q++ = '\t';
    const size_t mid_n = (size_t)(q - mid);
    q = w_i(ks, k); *q++ = '\t';
    const size_t ks_n = (size_t)(q - ks);
    q = w_u64(suf, qidx); *q++ = '\n';
    const size_t suf_n = (size_t)(q - suf);
    if (col_text.size() < target.size()) col_text.resize(target.size());
    for (uint64_t j = 0; j < cnt; j++) {
      const kmcpg_match& m = ms[j];
      std::string& ct = col_text[m.col];
      if (ct.empty()) {
        ct = target[m.col];
        ct.push_back('\t'); put_u64(ct, (uint16_t)m.target_idx);
        ct.push_back('\t'); put_u64(ct, m.target_idx >> 16);
        ct.push_back('\t'); put_u64(ct, m.gsize);
        ct.push_back('\t');
      }
      const std::string& f = fpr(qkmers, m.mkmers, m.fpr);
      if (pre_n + f.size() + ct.size() + 400 > LINE) {
        row(b, id, qlen, qkmers, cnt, target[m.col], m, k, qidx);
        continue;
      }
      char* p = line;
      memcpy(p, pre, pre_n); p += pre_n;
      memcpy(p, f.data(), f.size()); p += f.size(); *p++ = '\t';
      memcpy(p, mid, mid_n); p += mid_n;
      memcpy(p, ct.data(), ct.size()); p += ct.size();
      memcpy(p, ks, ks_n); p += ks_n;
      p = w_i(p, m.mkmers); *p++ = '\t';
      p = w_f4(p, m.qcov); *p++ = '\t';
      p = w_f4(p, m.tcov); *p++ = '\t';
      p = w_f4(p, m.jacc); *p++ = '\t';
      memcpy(p, suf, suf_n); p += suf_n;
      b.append(line, (size_t)(p - line));
    }
  }
  void unmatched(std::string& b, std::string_view id, int qlen, int qkmers, int k, uint64_t qidx) {
    b += id; b.push_back('\t'); put_i(b, qlen); b.push_back('\t'); put_i(b, qkmers);
    b += "\t0\t0\t\t-1\t0\t0\t"; put_i(b, k); b += "\t0\t0\t0\t0\t"; put_u64(b, qidx); b.push_back('\n');
  }
};

// Formatter threads that live as long as the run: each keeps its RowFormatter (and with it the cache of FPR strings, which
// a fresh formatter per batch would fill again and again).
class FormatPool {
 public:
  explicit FormatPool(int n) {
    for (int i = 0; i < n; i++) th_.emplace_back([this] { loop(); });
  }
  ~FormatPool() {
    {
      std::lock_guard<std::mutex> l(m_);
      stop_ = true;
      cv_.notify_all();
    }
    for (auto& t : th_) t.join();
  }
  // fn(part, formatter) for part = 0 .. parts-1, spread over the pool; returns when all are done
  void run(int parts, const std::function<void(int, RowFormatter&)>& fn) {
    std::unique_lock<std::mutex> l(m_);
    fn_ = &fn;
    next_ = 0;
    parts_ = parts;
    left_ = parts;
    cv_.notify_all();
    done_cv_.wait(l, [&] { return left_ == 0; });
    fn_ = nullptr;
  }

 private:
  void loop() {
    RowFormatter F;
    std::unique_lock<std::mutex> l(m_);
    for (;;) {
      cv_.wait(l, [&] { return stop_ || (fn_ && next_ < parts_); });
      if (stop_) return;
      const int pi = next_++;
      const auto* fn = fn_;
      l.unlock();
      (*fn)(pi, F);
      l.lock();
      if (--left_ == 0) done_cv_.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(int, RowFormatter&)>* fn_ = nullptr;
  int next_ = 0, parts_ = 0, left_ = 0;
  bool stop_ = false;
};
