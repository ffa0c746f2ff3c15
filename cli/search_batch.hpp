// search_batch.hpp — what kmcp-search's threads hand to one another (header only): a Batch of queries as the reader cuts it and the
// searchers and the writer pass it on, the bounded Queue between them, the two readers that cut input files into batches, and the
// geometry of sliding windows.  The including program provides die().
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include <sched.h>

#include "../include/kmcp_gpu.h"
#include "fastx_reader.hpp"

// Host cores this process may use: the affinity mask capped by the cgroup CPU quota (a GPU box shows 256 hardware threads and grants 16)
static inline unsigned usable_cpus() {
  unsigned n = std::max(1u, std::thread::hardware_concurrency());
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = (unsigned)std::max(1, CPU_COUNT(&set));
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[64];
    long long period = 0;
    if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) n = std::min<unsigned>(n, (unsigned)std::max(1ll, atoll(q) / period));
    fclose(f);
  }
  return n;
}

struct Batch {
  uint64_t seq = 0;  // position in the input: the writer emits batches in this order
  uint64_t n_seq = 1;  // how many of the reader's batches this one holds (batches read before the database was open are joined for a paged index)
  uint64_t first_idx = 0;
  std::vector<char> id_buf;  // query IDs back to back
  std::vector<uint64_t> id_offs{0};
  std::vector<uint8_t> seqs, seqs2;
  std::vector<uint64_t> offs{0}, offs2{0};
  kmcpg_result_summaries sres{};  // --regions-bed: one summary per window instead (kmcpg_wait_summaries)
  kmcpg_result_stats stats{};  // --ref-stats-only: what the batch came to, nothing else (kmcpg_wait_stats)
  std::vector<uint32_t> bins;   // --binning: one TaxId or KMCPG_BIN_NONE per query, and what the batch came to (kmcpg_wait_bins)
  kmcpg_result_bins bres{};
  kmcpg_result_pairs res{};  // compact result: (column, mKmers) pairs; the formatter threads expand a query's pairs right before its rows
  bool paired = false;
  // -g queries (whole files) are packed where the reader first touches their bases: 2-bit codes + the runs of other bytes
  // (kmcp_gpu.h kmcpg_pack2 / kmcpg_submit_packed); `seqs` stays empty, `offs` counts bases as ever
  bool packed = false;
  std::vector<uint8_t> codes;
  std::vector<kmcpg_exc_run> exc;  // size = capacity; n_exc of them are in use
  uint64_t n_exc = 0, n_bases = 0;
  void pack_append(const char* s, size_t n) {
    const size_t need = (size_t)((n_bases + n + 3) / 4 + 8);
    if (codes.size() < need) codes.resize(std::max(need, codes.size() + codes.size() / 2 + (1u << 20)));
    if (exc.size() < n_exc + 64) exc.resize(std::max<size_t>(1024, 2 * exc.size()));
    for (;;) {
      const uint64_t before = n_exc;
      const int rc = kmcpg_pack2((const uint8_t*)s, n, n_bases, codes.data(), exc.data(), exc.size(), &n_exc);
      if (rc == 0) break;
      if (rc != KMCPG_ENOMEM) die("%s", kmcpg_last_error());
      exc.resize(std::max<size_t>(2 * exc.size(), (size_t)n_exc + 1024));  // n_exc = how many runs there are in all
      n_exc = before;
    }
    n_bases += n;
  }
  // a whole query that was packed on its own (from base 0 of `src`): its codes are moved behind this batch's — a plain copy when the batch
  // ends on a byte, two shifts per byte otherwise — and its runs shifted to their place
  void append_packed(const uint8_t* src, uint64_t nb, const kmcpg_exc_run* runs, uint64_t n_runs) {
    const size_t need = (size_t)((n_bases + nb + 3) / 4 + 8);
    if (codes.size() < need) codes.resize(std::max(need, codes.size() + codes.size() / 2 + (1u << 20)));
    const size_t nbytes = (size_t)((nb + 3) / 4);
    const unsigned sh = 2u * (unsigned)(n_bases & 3);
    uint8_t* d = codes.data() + (n_bases >> 2);
    if (sh == 0) {
      memcpy(d, src, nbytes);
    } else {
      unsigned carry = d[0] & ((1u << sh) - 1u);
      for (size_t i = 0; i < nbytes; i++) {
        const unsigned v = src[i];
        d[i] = (uint8_t)(carry | (v << sh));
        carry = v >> (8 - sh);
      }
      d[nbytes] = (uint8_t)carry;
    }
    if (exc.size() < n_exc + n_runs) exc.resize(std::max<size_t>((size_t)(n_exc + n_runs), 2 * exc.size()));
    for (uint64_t i = 0; i < n_runs; i++) exc[n_exc + i] = kmcpg_exc_run{runs[i].pos + n_bases, runs[i].len, runs[i].byte};
    n_exc += n_runs;
    n_bases += nb;
  }
  // sliding windows: the records' windows are the batch's queries — wpre[r] = windows of records 0 .. r-1, res has one row per window
  bool windows = false;
  std::vector<uint64_t> wpre{0};
  uint64_t bases() const { return packed ? n_bases : (uint64_t)(seqs.size() + seqs2.size()); }
  size_t size() const { return id_offs.size() - 1; }
  std::string_view id(size_t i) const { return std::string_view(id_buf.data() + id_offs[i], (size_t)(id_offs[i + 1] - id_offs[i])); }
  // the queries of `o` (the reader's next batch) behind this one's
  void append(const Batch& o) {
    const uint64_t ib = id_buf.size(), sb = seqs.size(), sb2 = seqs2.size();
    id_buf.insert(id_buf.end(), o.id_buf.begin(), o.id_buf.end());
    for (size_t i = 1; i < o.id_offs.size(); i++) id_offs.push_back(ib + o.id_offs[i]);
    seqs.insert(seqs.end(), o.seqs.begin(), o.seqs.end());
    for (size_t i = 1; i < o.offs.size(); i++) offs.push_back(sb + o.offs[i]);
    if (paired) {
      seqs2.insert(seqs2.end(), o.seqs2.begin(), o.seqs2.end());
      for (size_t i = 1; i < o.offs2.size(); i++) offs2.push_back(sb2 + o.offs2[i]);
    }
    n_seq += o.n_seq;
  }
};

template <typename T>
class Queue {
 public:
  explicit Queue(size_t cap) : cap_(cap) {}
  void push(T v) {
    std::unique_lock<std::mutex> l(m_);
    cv_.wait(l, [&] { return q_.size() < cap_; });
    q_.push_back(std::move(v));
    cv_.notify_all();
  }
  bool pop(T* v) {
    std::unique_lock<std::mutex> l(m_);
    cv_.wait(l, [&] { return !q_.empty() || closed_; });
    if (q_.empty()) return false;
    *v = std::move(q_.front());
    q_.pop_front();
    cv_.notify_all();
    return true;
  }
  bool try_pop(T* v) {  // what is there right now, without waiting
    std::lock_guard<std::mutex> l(m_);
    if (q_.empty()) return false;
    *v = std::move(q_.front());
    q_.pop_front();
    cv_.notify_all();
    return true;
  }
  void close() {
    std::lock_guard<std::mutex> l(m_);
    closed_ = true;
    cv_.notify_all();
  }

 private:
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<T> q_;
  size_t cap_;
  bool closed_ = false;
};

// The records of one single-end input file as batches of about `batch_reads` queries, in file order.  Plain four-line FASTQ
// files are cut and parsed by several threads (ParallelFastq: every chunk becomes a batch without another copy); everything
// else — gzip, BGZF, FASTA, wrapped FASTQ, pipes — goes through the single-threaded FastxReader.  Returns the number of records.
// `stop` (optional) is looked at between batches / records: once set the rest of the file is left unread.
template <class Emit>
static uint64_t read_single_end(const std::string& file, size_t batch_reads, size_t max_bases, Emit&& emit, const std::atomic<bool>* stop = nullptr) {
  uint64_t n = 0;
  std::unique_ptr<Batch> b(new Batch());
  auto flush = [&] {
    if (b->size() == 0) return;
    n += b->size();
    emit(std::move(b));
    b.reset(new Batch());
  };
  auto add = [&](const FastxRec& r) {
    b->id_buf.insert(b->id_buf.end(), r.id, r.id + r.id_len);
    b->id_offs.push_back(b->id_buf.size());
    b->seqs.insert(b->seqs.end(), (const uint8_t*)r.seq, (const uint8_t*)r.seq + r.seq_len);
    b->offs.push_back(b->seqs.size());
    if (b->size() >= batch_reads || b->seqs.size() >= max_bases) flush();
  };
  uint64_t resume = 0;
  bool serial = true;
  if (ParallelFastq::eligible(file)) {
    int w = (int)std::min(8u, std::max(2u, usable_cpus() / 2));
    if (const char* e = getenv("KMCP_READER_THREADS")) w = std::max(1, atoi(e));
    ParallelFastq pf(file, batch_reads, w, 2 * max_bases);  // a record is its bases twice (qualities) plus the header
    serial = false;
    while (std::unique_ptr<FastqChunk> c = pf.next()) {
      if (stop && stop->load(std::memory_order_relaxed)) return n;
      if (!c->strict) {  // not four-line FASTQ from here on: the general reader takes over at the chunk's first byte
        resume = c->file_off;
        serial = true;
        break;
      }
      if (c->size() == 0) continue;
      std::unique_ptr<Batch> cb(new Batch());
      cb->id_buf.swap(c->id_buf);
      cb->id_offs.swap(c->id_offs);
      cb->seqs.swap(c->seqs);
      cb->offs.swap(c->offs);
      n += cb->size();
      emit(std::move(cb));
    }
  }
  if (serial) {
    FastxReader r(file, resume);
    FastxRec rec;
    while (!(stop && stop->load(std::memory_order_relaxed)) && r.next(&rec)) add(rec);
    if (!(stop && stop->load(std::memory_order_relaxed))) flush();
  }
  return n;
}

// The records of two mate files as batches of pairs (IDs of read 1), in file order; ends with the shorter file, like the
// reference's loop (search.go:807-826).  Both files go through read_single_end — several parser threads each for plain FASTQ —
// the mates on a thread of their own; read 2's batches are re-cut at read 1's batch boundaries (buffers are taken over
// without a copy where the boundaries agree, which they do for reads of equal length).  Returns the number of pairs.
template <class Emit>
static uint64_t read_paired(const std::string& file1, const std::string& file2, size_t batch_reads, size_t max_bases, Emit&& emit) {
  Queue<std::unique_ptr<Batch>> q2(4);
  // the pairs end with the shorter file (search.go:807-826): whichever reader is still going when the other file is exhausted
  // stops at its next batch instead of parsing the rest of a file nobody will look at
  std::atomic<bool> ended{false}, stop2{false};
  std::thread mate_reader([&] {
    read_single_end(file2, batch_reads, std::max<size_t>(1, max_bases / 2), [&](std::unique_ptr<Batch> b) { q2.push(std::move(b)); }, &stop2);
    q2.close();
  });
  std::unique_ptr<Batch> cur;  // the batch of read 2 being consumed
  size_t ci = 0;               // records of it already handed out
  uint64_t n = 0;
  read_single_end(file1, batch_reads, std::max<size_t>(1, max_bases / 2), [&](std::unique_ptr<Batch> b) {
    if (ended) return;
    const size_t want = b->size();
    size_t have = 0;
    b->paired = true;
    while (have < want) {
      if (!cur || ci == cur->size()) {
        ci = 0;
        cur.reset();
        if (!q2.pop(&cur)) {
          ended = true;
          break;
        }
        continue;
      }
      if (have == 0 && ci == 0 && cur->size() == want) {
        b->seqs2.swap(cur->seqs);
        b->offs2.swap(cur->offs);
        cur.reset();
        have = want;
        break;
      }
      const size_t take = std::min(want - have, cur->size() - ci);
      const uint64_t lo = cur->offs[ci], hi = cur->offs[ci + take], base = b->seqs2.size();
      b->seqs2.insert(b->seqs2.end(), cur->seqs.begin() + (ptrdiff_t)lo, cur->seqs.begin() + (ptrdiff_t)hi);
      for (size_t i = 1; i <= take; i++) b->offs2.push_back(base + (cur->offs[ci + i] - lo));
      ci += take;
      have += take;
    }
    if (have < want) {  // read 2 ended inside this batch
      b->id_buf.resize((size_t)b->id_offs[have]);
      b->id_offs.resize(have + 1);
      b->seqs.resize((size_t)b->offs[have]);
      b->offs.resize(have + 1);
    }
    if (have == 0) return;
    n += have;
    emit(std::move(b));
  }, &ended);
  stop2 = true;            // read 1 ended first (or both did): the mates' thread stops at its next batch
  while (q2.pop(&cur)) {}  // ... and is not left blocked on a full queue
  mate_reader.join();
  return n;
}

// Sliding windows, as `seqkit sliding -s step -W window [-g]` cuts a record of L bases: window j starts at base j * step and holds `window`
// bases; with greedy the windows go on while they start inside the record and are cut at its end, without it they stop at the first one
// that would run over.  The library states the same (kmcp_gpu.h kmcpg_window_count / kmcpg_window_locate; tests/window_geometry_check.cpp
// holds the two against each other).
static inline uint64_t window_count(uint64_t L, const kmcpg_window_spec& spec) {
  if (L == 0) return 0;
  if (spec.greedy) return (L + spec.step - 1) / spec.step;
  return L >= spec.window ? (L - spec.window) / spec.step + 1 : 0;
}
struct WindowSpan {
  uint64_t start, end;  // bases start .. end - 1 of the record (0-based)
};
static inline WindowSpan window_span(uint64_t L, uint64_t j, const kmcpg_window_spec& spec) {
  const uint64_t start = j * spec.step;
  return {start, std::min<uint64_t>(start + spec.window, L)};
}
