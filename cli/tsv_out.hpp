// tsv_out.hpp — what the host-only TSV commands (kmcp-merge, kmcp-filter) share: the fatal-error exit of the reference's checkError and
// the output writer (plain, or gzip members compressed side by side).
#pragma once
#include <zlib.h>

#include <algorithm>
#include <cerrno>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace tsv_out {

[[noreturn]] inline void die(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "[ERRO] ");
  vfprintf(stderr, fmt, ap);
  fputc('\n', stderr);
  va_end(ap);
  exit(255);  // checkError: os.Exit(-1)
}

// The output: plain, or gzip written as a sequence of members (1 MB of text each) that a few threads compress side by side —
// what the reference gets from pgzip; gzip readers, `kmcp profile` included, read the members as one stream.
struct Out {
  FILE* fp = nullptr;
  bool gz = false;
  int level = 6;
  std::string buf;
  struct Job {
    std::string in, out;
    bool done = false;
  };
  std::deque<std::shared_ptr<Job>> order_, todo_;
  std::vector<std::thread> workers_;
  std::mutex m_;
  std::condition_variable cv_;
  bool stop_ = false;

  Out(const std::string& path, int level_) {
    gz = path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0;
    level = level_ < 0 ? 6 : std::min(level_, 9);
    fp = path == "-" ? stdout : fopen(path.c_str(), "wb");
    if (!fp) die("%s: %s", path.c_str(), strerror(errno));
    buf.reserve(1 << 20);
    if (gz) {
      const unsigned n = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
      for (unsigned i = 0; i < n; i++) workers_.emplace_back([this] { work(); });
    }
  }
  ~Out() {
    {
      std::lock_guard<std::mutex> l(m_);
      stop_ = true;
      cv_.notify_all();
    }
    for (auto& t : workers_) t.join();
  }
  static void gzip_member(const std::string& in, int level, std::string* out) {
    z_stream z{};
    if (deflateInit2(&z, level, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) die("zlib: deflateInit2 failed");
    out->resize(deflateBound(&z, (uLong)in.size()) + 64);
    z.next_in = (Bytef*)in.data();
    z.avail_in = (uInt)in.size();
    z.next_out = (Bytef*)&(*out)[0];
    z.avail_out = (uInt)out->size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) die("zlib: deflate failed");
    out->resize(z.total_out);
    deflateEnd(&z);
  }
  void work() {
    for (;;) {
      std::shared_ptr<Job> j;
      {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return stop_ || !todo_.empty(); });
        if (todo_.empty()) return;
        j = std::move(todo_.front());
        todo_.pop_front();
      }
      gzip_member(j->in, level, &j->out);
      std::lock_guard<std::mutex> l(m_);
      j->done = true;
      cv_.notify_all();
    }
  }
  void put(const char* p, size_t n) {
    if (n && fwrite(p, 1, n, fp) != n) die("write error");
  }
  // writes the members that are ready, in order; with `all` waits for every one of them
  void drain(bool all) {
    std::unique_lock<std::mutex> l(m_);
    for (;;) {
      if (order_.empty()) return;
      if (!order_.front()->done) {
        if (!all && order_.size() < 4 * workers_.size()) return;
        cv_.wait(l, [&] { return order_.front()->done; });
      }
      std::shared_ptr<Job> j = std::move(order_.front());
      order_.pop_front();
      l.unlock();
      put(j->out.data(), j->out.size());
      l.lock();
    }
  }
  void flush() {
    if (buf.empty()) return;
    if (gz) {
      std::shared_ptr<Job> j(new Job());
      members_++;
      j->in.swap(buf);
      buf.reserve(1 << 20);
      {
        std::lock_guard<std::mutex> l(m_);
        order_.push_back(j);
        todo_.push_back(j);
        cv_.notify_all();
      }
      drain(false);
    } else {
      put(buf.data(), buf.size());
      buf.clear();
    }
  }
  void write(const char* p, size_t n) {
    buf.append(p, n);
    if (buf.size() > (1u << 20) - 4096) flush();
  }
  void write(const std::string& s) { write(s.data(), s.size()); }
  // a result line with its hits field [lo, hi) replaced, and a newline
  void write_row(const char* line, size_t lo, size_t hi, size_t len, const char* hits, size_t hn) {
    const size_t at = buf.size(), n = lo + hn + (len - hi) + 1;
    buf.resize(at + n);
    char* d = &buf[at];
    memcpy(d, line, lo);
    memcpy(d + lo, hits, hn);
    memcpy(d + lo + hn, line + hi, len - hi);
    d[n - 1] = '\n';
    if (buf.size() > (1u << 20) - 4096) flush();
  }
  void write(const char* s) { write(s, strlen(s)); }
  void close() {
    flush();
    if (gz) {
      drain(true);
      if (members_ == 0) {  // an empty .gz is still a gzip file
        std::string e;
        gzip_member(std::string(), level, &e);
        put(e.data(), e.size());
      }
    }
    if (fp != stdout) {
      if (fclose(fp) != 0) die("write error");
    } else fflush(fp);
    fp = nullptr;
  }
  size_t members_ = 0;
};

}  // namespace tsv_out
