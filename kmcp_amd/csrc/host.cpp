// host.cpp — what is above a lane (lane.hpp) in the pipeline on host buffers: a ticket over the handle's GPUs (submit_impl), the host half
// of a wait (finish_raw), the retry walk of --try-se and of multi-k databases (retry_unmatched), the pieces and the ENOMEM halves of
// kmcpg_search_batch, the host half of a summary ticket (finish_summary: K5's records, the windows it left), and the submit / wait / search
// entries with kmcpg_batch_hint.
// Reference counterparts: handleQuery (util-db-search.go:763-1025), :831-850, :1001-1014.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "exchange.hpp"
#include "k3_set_order.hpp"
#include "lane.hpp"
#include "regions_rule.hpp"
#include "specific_rule.hpp"

namespace kmcpg {

int submit_impl(kmcpg_db* db, const HostBatch& b, const kmcpg_params& p, bool retry, bool block, kmcpg_ticket** out, const PackedIn* packed, bool summary, bool stats, bool bins) {
  std::unique_ptr<kmcpg_ticket> t(new kmcpg_ticket());
  t->db = db;
  t->n = b.n;
  t->paired = b.seqs2 != nullptr;
  t->p = p;
  t->summary = summary;
  t->stats = stats;
  t->bins = bins;
  if (db->paged_passes > 0) {
    int rc = search_paged(db, b, p, t.get());
    if (rc) return rc;
    *out = t.release();
    return 0;
  }
  std::vector<kmcpg_db*> targets = db->shards.empty() ? std::vector<kmcpg_db*>{db} : db->shards;
  for (kmcpg_db* sh : targets) {
    AsyncState* A = nullptr;
    int rc = async_state(sh, &A);
    if (rc) {
      drop_ticket(t.release(), true);
      return rc;
    }
    Lane* lane = acquire_lane(A, retry, block);
    if (!lane) {
      drop_ticket(t.release());
      return fail_all_lanes_busy(A);
    }
    t->parts.push_back({sh, lane, retry});
  }
  // every GPU gets the whole batch (150 B per read; cheaper than moving k-mer hashes between GPUs)
  std::vector<int> rcs(t->parts.size(), 0);
  std::vector<std::string> errs(t->parts.size());
  // text may go up as 2-bit codes where nothing reads the staged ASCII again: single reads (never pairs), no retry sub-batch, no smaller k to come
  const bool can_pack = !b.seqs2 && !retry && !rereads_text(db, p);
  auto one = [&](size_t i) {
    auto& pt = t->parts[i];
    rcs[i] = packed ? stage_packed(pt.lane, *packed, b) : stage(pt.lane, b, can_pack);
    if (rcs[i] == 0) pt.lane->summary = summary, pt.lane->stats = stats, pt.lane->bins = bins;
    if (rcs[i] == 0) rcs[i] = enqueue(pt.shard, pt.shard->async, pt.lane, p);
    if (rcs[i]) errs[i] = kmcpg_err_ref();
  };
  if (t->parts.size() == 1) one(0);
  else {
    std::vector<std::thread> th;
    for (size_t i = 0; i < t->parts.size(); i++) th.emplace_back(one, i);
    for (auto& x : th) x.join();
  }
  for (size_t i = 0; i < rcs.size(); i++)
    if (rcs[i]) {
      const int rc = rcs[i];
      const std::string msg = t->parts.size() > 1 ? "device " + std::to_string(t->parts[i].shard->opts.device) + ": " + errs[i] : errs[i];
      drop_ticket(t.release(), true);
      return kmcpg_fail(rc, "%s", msg.c_str());
    }
  Lane* L0 = t->parts[0].lane;
  t->S[0] = L0->h_seqs.p;
  t->O[0] = L0->h_offs.p;
  t->S[1] = t->paired ? L0->h_seqs2.p : nullptr;
  t->O[1] = t->paired ? L0->h_offs2.p : nullptr;
  *out = t.release();
  return 0;
}

namespace {

// raw results of a ticket -> finalized matches (host half).  The hit lists of the parts are concatenated exactly as the
// reference concatenates the replies of its per-block workers (:946-964).
int finish_raw(kmcpg_ticket* t, kmcpg_result* out, bool as_pairs) {
  const kmcpg_hit* hits = nullptr;
  uint64_t n_hits = 0;
  static thread_local std::vector<kmcpg_hit, NoInitAlloc<kmcpg_hit>> merged;
  if (t->paged)
    return kmcpg_finalize(t->db, t->hits.data(), t->hits.size(), t->n ? t->qk.data() : nullptr, t->n ? t->ql.data() : nullptr, t->n, &t->p, out);
  if (t->parts.size() == 1 && !t->db->exchange) {
    auto& pt = t->parts[0];
    int rc = collect(pt.shard, pt.shard->async, pt.lane, t->p, &n_hits);
    if (rc) return rc;
    if (pt.lane->grouped && t->n)
      return finalize_grouped_trusted(t->db, pt.lane->h_pairs.p, pt.lane->h_roffs.p, pt.lane->h_qk.p, pt.lane->h_ql.p, t->n, t->p, out, pt.lane->bound_n, as_pairs,
                                      pt.lane->spec ? pt.lane->h_verd.p : nullptr);
    hits = pt.lane->h_hits.p;
  } else if (Exchange* x = t->db->exchange) {
    // the shards' lists meet on the first GPU (RCCL send/recv over xGMI, exactly the bytes each shard produced) and come to
    // the host in one copy
    std::vector<const void*> src;
    std::vector<uint64_t> bytes;
    for (auto& pt : t->parts) {
      uint64_t c = 0;
      int rc = collect(pt.shard, pt.shard->async, pt.lane, t->p, &c, false);
      if (rc) return kmcpg_fail(rc, "device %d: %s", pt.shard->opts.device, std::string(kmcpg_err_ref()).c_str());
      src.push_back(pt.lane->d_hits.p);
      bytes.push_back(c * sizeof(kmcpg_hit));
      n_hits += c;
    }
    Lane* L0 = t->parts[0].lane;
    kmcpg_db* sh0 = t->parts[0].shard;
    if (hipSetDevice(sh0->opts.device) != hipSuccess) return kmcpg_fail(KMCPG_EDEVICE, "hipSetDevice failed");
    if (sh0->async->device_finalize && t->n && n_hits) {
      // K3 on the gathering GPU, over the concatenation of all shards' lists (every shard knows every column's k-mer count):
      // grouped by read, filtered by -T, in final order; 8 bytes per match and the reads' offsets come to the host
      if (L0->d_pairs.ensure(n_hits) || L0->d_roffs.ensure((size_t)t->n + 2) || L0->h_roffs.ensure((size_t)t->n + 2))
        return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
      uint64_t* h_word = L0->h_cnt.p;  // pinned; the lane's counters have been read by collect()
      h_word[0] = n_hits;
      const kmcpg_params p = t->p;
      const uint32_t n = t->n;
      int rc = exchange_gather(x, src, bytes, nullptr, [&](uint8_t* d_cat, uint64_t, void* st) -> int {
        uint64_t* d_word = (uint64_t*)(d_cat - 16);
        HIPCHK(hipMemcpyAsync(d_word, h_word, sizeof(uint64_t), hipMemcpyHostToDevice, (hipStream_t)st));
        int rc2 = kmcpg_group_device(sh0, (const kmcpg_hit*)d_cat, d_word, n_hits, L0->d_qk.p, n, &p, L0->d_pairs.p, L0->d_roffs.p, st);
        if (rc2) return rc2;
        HIPCHK(hipMemcpyAsync(L0->h_roffs.p, L0->d_roffs.p, ((size_t)n + 2) * sizeof(uint64_t), hipMemcpyDeviceToHost, (hipStream_t)st));
        // only what survived -T comes down: the offsets first (nobody else's gather is held up by this wait: the exchange mutex is
        // not held here), then h_roffs[n] pairs, as collect() does on the single-GPU path
        HIPCHK(hipStreamSynchronize((hipStream_t)st));
        const uint64_t kept = std::min<uint64_t>(L0->h_roffs.p[n], n_hits);
        if (L0->h_pairs.ensure(kept + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
        if (kept) HIPCHK(hipMemcpyAsync(L0->h_pairs.p, L0->d_pairs.p, kept * sizeof(kmcpg_pair), hipMemcpyDeviceToHost, (hipStream_t)st));
        return 0;
      });
      if (rc) return rc;
      int32_t bound_n = INT32_MAX;  // every shard ran the same params on the same batch; the smallest cover is what holds for the merged list
      for (auto& pt : t->parts) bound_n = std::min(bound_n, pt.lane->bound_n);
      return finalize_grouped_trusted(t->db, L0->h_pairs.p, L0->h_roffs.p, L0->h_qk.p, L0->h_ql.p, t->n, t->p, out, bound_n, as_pairs);
    }
    if (L0->h_hits.ensure(n_hits + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
    int rc = exchange_gather(x, src, bytes, (uint8_t*)L0->h_hits.p);
    if (rc) return rc;
    hits = L0->h_hits.p;
  } else {
    merged.clear();
    for (auto& pt : t->parts) {
      uint64_t c = 0;
      int rc = collect(pt.shard, pt.shard->async, pt.lane, t->p, &c);
      if (rc) return kmcpg_fail(rc, "device %d: %s", pt.shard->opts.device, std::string(kmcpg_err_ref()).c_str());
      merged.insert(merged.end(), pt.lane->h_hits.p, pt.lane->h_hits.p + c);
    }
    hits = merged.data();
    n_hits = merged.size();
  }
  Lane* L0 = t->parts[0].lane;  // every shard generates the same k-mers
  int rcf = kmcpg_finalize(t->db, hits, n_hits, t->n ? L0->h_qk.p : nullptr, t->n ? L0->h_ql.p : nullptr, t->n, &t->p, out);
  // the counting stages without K3 in front of them (KMCPG_DEVICE_FINALIZE=0): every read, from the finished (unfiltered) records
  if (rcf == 0) counting_host_result(t->db, out);
  // the species-specific stage without K3 in front of it (KMCPG_DEVICE_FINALIZE=0): the rule on the finished records
  if (rcf == 0 && t->db->spec_on()) specific_filter_result(t->db, out);
  return rcf;
}

// gives the ticket back; after a failure its lanes are drained first and the error text stays the failure's
void drop_after(kmcpg_ticket* t, int rc) {
  if (rc) keeping_error([&] { drop_ticket(t, true); });
  else drop_ticket(t);
}

// a small synchronous search on the retry lane(s): the sub-batches of --try-se and of the smaller k of multi-k databases
// (always Match records: retry_unmatched splices them into the batch's result record by record)
int search_sync(kmcpg_db* db, const HostBatch& b, const kmcpg_params& p, kmcpg_result* out) {
  kmcpg_ticket* t = nullptr;
  int rc = submit_impl(db, b, p, true, true, &t);
  if (rc) return rc;
  rc = finish_raw(t, out, false);
  drop_after(t, rc);
  return rc;
}

// What the reference does with a query that was searched but matched nothing (handleQuery, util-db-search.go:763-1025):
// with --try-se the k-mers of read 1, then of read 2 are searched on their own (:831-850, :1001-1014; the length gate is not
// applied again); if the database holds several k-mer sizes the whole procedure is repeated with the next smaller k
// (:764, :1016-1022).  A query with fewer than MinMatched k-mers at any step is final (:854-869).
int retry_unmatched(kmcpg_ticket* t, kmcpg_result* out) {
  kmcpg_db* db = t->db;
  const kmcpg_params& p = t->p;
  const uint32_t n = t->n;
  if (n == 0 || !may_retry(db, p, t->paired)) return 0;
  std::vector<int> ks = db->ks_desc;  // descending
  if (p.k > 0) ks.assign(1, p.k);     // an explicit k: no walk over the database's sizes
  const bool try_se = p.try_se && t->paired;
  ResultOwner* o = (ResultOwner*)out->owner;
  const uint8_t* S[2] = {t->S[0], t->S[1]};  // the batch as staged
  const uint64_t* O[2] = {t->O[0], t->O[1]};
  std::vector<char> final_(n, 0);
  std::vector<uint32_t> todo;
  std::vector<uint8_t> sub[2];
  std::vector<uint64_t> so[2];
  // splices the result of a sub-batch (queries `todo`) into the batch result
  auto splice = [&](const kmcpg_result& r2, bool whole_query, int k) {
    std::vector<uint64_t> noffs((size_t)n + 1, 0);
    MatchVec nm;
    size_t ti = 0;
    for (uint32_t r = 0; r < n; r++) {
      if (ti < todo.size() && todo[ti] == r) {
        o->qlen[r] = r2.qlen[ti];
        o->ksize[r] = k;
        if (r2.qkmers[ti] > 0) o->qkmers[r] = r2.qkmers[ti];
        else {
          final_[r] = 1;  // fewer than MinMatched k-mers: the reference returns here (:854-869)
          if (whole_query) o->qkmers[r] = 0;  // a fresh QueryResult: NumKmers never set (this build reports 0)
        }
        if (r2.match_offs[ti + 1] > r2.match_offs[ti]) final_[r] = 1;
        nm.insert(nm.end(), r2.matches + r2.match_offs[ti], r2.matches + r2.match_offs[ti + 1]);
        ti++;
      } else {
        nm.insert(nm.end(), o->matches.begin() + (ptrdiff_t)o->offs[r], o->matches.begin() + (ptrdiff_t)o->offs[r + 1]);
      }
      noffs[r + 1] = nm.size();
    }
    o->matches.swap(nm);
    o->offs.swap(noffs);
  };
  // after the first pass: matched, or never searched (too short / fewer than MinMatched k-mers) => final
  for (uint32_t r = 0; r < n; r++) final_[r] = (o->offs[r + 1] > o->offs[r]) || o->qkmers[r] <= 0;
  int rc = 0;
  for (size_t ik = 0; ik < ks.size() && rc == 0; ik++) {
    if (ik > 0) {  // the whole query again with the next smaller k
      todo.clear();
      for (uint32_t r = 0; r < n; r++)
        if (!final_[r]) todo.push_back(r);
      if (todo.empty()) break;
      for (int m = 0; m < 2; m++) {
        sub[m].clear();
        so[m].assign(1, 0);
        if (!S[m]) continue;
        for (uint32_t r : todo) {
          sub[m].insert(sub[m].end(), S[m] + O[m][r], S[m] + O[m][r + 1]);
          so[m].push_back(sub[m].size());
        }
      }
      kmcpg_params q = p;
      q.k = ks[ik];
      q.try_se = 0;
      kmcpg_result r2;
      rc = search_sync(db, HostBatch{sub[0].data(), so[0].data(), S[1] ? sub[1].data() : nullptr, S[1] ? so[1].data() : nullptr, (uint32_t)todo.size()}, q, &r2);
      if (rc) break;
      splice(r2, true, ks[ik]);
      kmcpg_result_free(&r2);
    }
    if (!try_se) continue;
    for (int mate = 0; mate < 2 && rc == 0; mate++) {
      todo.clear();
      for (uint32_t r = 0; r < n; r++)
        if (!final_[r]) todo.push_back(r);
      if (todo.empty()) break;
      sub[0].clear();
      so[0].assign(1, 0);
      for (uint32_t r : todo) {
        sub[0].insert(sub[0].end(), S[mate] + O[mate][r], S[mate] + O[mate][r + 1]);
        so[0].push_back(sub[0].size());
      }
      kmcpg_params q = p;
      q.k = ks[ik];
      q.min_qlen = 0;  // the length gate was applied once, before k-mer generation
      q.try_se = 0;
      kmcpg_result r2;
      rc = search_sync(db, HostBatch{sub[0].data(), so[0].data(), nullptr, nullptr, (uint32_t)todo.size()}, q, &r2);
      if (rc) break;
      splice(r2, false, ks[ik]);
      kmcpg_result_free(&r2);
    }
  }
  out->qlen = o->qlen.data();
  out->qkmers = o->qkmers.data();
  out->ksize = o->ksize.data();
  out->matches = o->matches.data();
  out->match_offs = o->offs.data();
  return rc;
}

}  // namespace

void concat_results(const kmcpg_db* db, kmcpg_result* parts, size_t np, uint32_t n, bool as_pairs, int k_used, kmcpg_result* out) {
  ResultOwner* o = result_owner_take();
  result_owner_shape(o, n, as_pairs);
  uint32_t base = 0;
  std::vector<kmcpg_match> ex;
  for (size_t i = 0; i < np; i++) {
    kmcpg_result& r = parts[i];
    ResultOwner* oi = (ResultOwner*)r.owner;
    const uint32_t m = r.n_reads;
    if (oi && m) {
      if (o->pairs_mode) result_records_to_pairs(oi);
      for (uint32_t q = 0; q < m; q++) {
        o->qlen[base + q] = r.qlen[q];
        o->qkmers[base + q] = r.qkmers[q];
        o->ksize[base + q] = r.ksize[q];
        const uint64_t a = oi->offs[q], b = oi->offs[q + 1];
        o->offs[(size_t)base + q + 1] = b - a;
        if (o->pairs_mode) o->pairs.insert(o->pairs.end(), oi->pairs.begin() + (ptrdiff_t)a, oi->pairs.begin() + (ptrdiff_t)b);
        else if (!oi->pairs_mode) o->matches.insert(o->matches.end(), oi->matches.begin() + (ptrdiff_t)a, oi->matches.begin() + (ptrdiff_t)b);
        else {  // (a part finished in the compact form, the caller wants records)
          ex.resize(b - a);
          if (b > a) (void)kmcpg_expand_pairs(db, r.qkmers[q], oi->pairs.data() + a, b - a, ex.data());
          o->matches.insert(o->matches.end(), ex.begin(), ex.end());
        }
      }
    }
    base += m;
    kmcpg_result_free(&r);
  }
  result_publish(o, n, k_used, out);
}

int wait_impl(kmcpg_ticket* t, kmcpg_result* out, bool as_pairs) {
  memset(out, 0, sizeof *out);
  int rc;
  if (!t->pieces.empty()) rc = wait_pieces(t, out, as_pairs);
  else {
    rc = finish_raw(t, out, as_pairs);
    if (rc == 0) rc = retry_unmatched(t, out);
  }
  if (rc) kmcpg_result_free(out);
  drop_after(t, rc);
  return rc;
}

namespace {

// the summary of reads [0, r.n_reads) of a finished result of Match records (their final rows, in print order) by the rule of
// regions_rule.hpp over target_class; x = the qCov as "%.4f" prints it, parsed back (k3_set_order.hpp fixed4) — the operations of K5
void summaries_of_records(const kmcpg_db* db, const kmcpg_result& r, kmcpg_window_summary* s) {
  const uint32_t* const cls = db->h_spec_target.data();
  WindowSummaryAcc acc;
  for (uint32_t i = 0; i < r.n_reads; i++) {
    acc.clear();
    for (uint64_t j = r.match_offs[i]; j < r.match_offs[i + 1]; j++) acc.add(cls[r.matches[j].col], (double)fixed4(r.matches[j].qcov) / 10000.0);
    s[i] = kmcpg_window_summary{acc.n, 0u, acc.n ? acc.score() : 0.0};
  }
}

// one batch of a summary ticket.  K5 ran behind K4 (Lane::summarized): the records are here; the windows it LEFT — several targets among
// more than K5_CAP pairs, and those whose pairs the host's -f test may still thin out — get their pairs now and go through the host half
// as a small batch of their own.  Every other path (no K3: KMCPG_DEVICE_FINALIZE=0) finishes the records and summarises those.
int finish_summary(kmcpg_ticket* t, SummaryPart* out) {
  const uint32_t n = t->n;
  out->s.assign(n, kmcpg_window_summary{});
  out->qlen.assign(n, 0);
  out->qkmers.assign(n, 0);
  if (n == 0) return 0;
  auto& pt = t->parts[0];
  Lane* L = pt.lane;
  if (t->paged || t->parts.size() != 1 || t->db->exchange || !L->summarized()) {
    kmcpg_result r{};
    if (int rc = finish_raw(t, &r, false)) return rc;
    summaries_of_records(t->db, r, out->s.data());
    memcpy(out->qlen.data(), r.qlen, (size_t)n * sizeof(int32_t));
    memcpy(out->qkmers.data(), r.qkmers, (size_t)n * sizeof(int32_t));
    for (uint32_t i = 0; i < n; i++)
      if (r.match_offs[i + 1] > r.match_offs[i]) out->left++, out->left_pairs += r.match_offs[i + 1] - r.match_offs[i];  // all of them the host's
      else out->empty++;
    kmcpg_result_free(&r);
    return 0;
  }
  uint64_t n_hits = 0;
  if (int rc = collect(pt.shard, pt.shard->async, L, t->p, &n_hits, false)) return rc;
  if (L->h_roffs.p[(size_t)n + 1] != 0)
    return kmcpg_fail(KMCPG_EINVAL, "%llu hit(s) named a read or column that does not exist", (unsigned long long)L->h_roffs.p[(size_t)n + 1]);
  memcpy(out->s.data(), L->h_sum.p, (size_t)n * sizeof(kmcpg_window_summary));
  memcpy(out->qlen.data(), L->h_ql.p, (size_t)n * sizeof(int32_t));
  memcpy(out->qkmers.data(), L->h_qk.p, (size_t)n * sizeof(int32_t));
  out->bytes_d2h = (uint64_t)n * (sizeof(kmcpg_window_summary) + 2 * sizeof(int32_t)) + 4 * sizeof(uint64_t);  // + K2's two counters, K3's two last words
  // the LEFT windows: a record carries the segment's length (n_targets) and whether the host still judges it
  std::vector<uint32_t> idx;
  std::vector<uint64_t> offs(1, 0);
  for (uint32_t i = 0; i < n; i++)
    if (out->s[i].flags & KMCPG_SUMMARY_LEFT) {
      idx.push_back(i);
      offs.push_back(offs.back() + out->s[i].n_targets);
    } else (out->s[i].n_targets == 0 ? out->empty : out->s[i].n_targets == 1 ? out->single : out->wave)++;
  out->left = idx.size();
  if (idx.empty()) return 0;
  const uint64_t total = offs.back();
  if (total > L->h_roffs.p[n] || total > L->d_pairs.cap) return kmcpg_fail(KMCPG_EDEVICE, "internal: K5 left %llu pairs of %llu", (unsigned long long)total, (unsigned long long)L->h_roffs.p[n]);
  if (L->h_pairs.ensure(total)) return kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
  {
    kmcpg_db* sh = pt.shard;
    KMCPG_USE_DEVICE(sh);
    HIPCHK(hipMemcpyAsync(L->h_pairs.p, L->d_final, total * sizeof(kmcpg_pair), hipMemcpyDeviceToHost, sh->async->copy_stream));
    HIPCHK(hipStreamSynchronize(sh->async->copy_stream));
  }
  out->left_pairs = total;
  out->bytes_d2h += total * sizeof(kmcpg_pair);
  const uint32_t nl = (uint32_t)idx.size();
  offs.push_back(0);  // (the word behind the offsets: no bad hits)
  std::vector<int32_t> qk(nl), ql(nl);
  std::vector<uint8_t> verd(nl);
  for (uint32_t j = 0; j < nl; j++) {
    qk[j] = out->qkmers[idx[j]];
    ql[j] = out->qlen[idx[j]];
    verd[j] = out->s[idx[j]].flags & KMCPG_SUMMARY_HOST ? SPECIFIC_HOST : SPECIFIC_KEEP;
  }
  kmcpg_result r{};
  if (int rc = finalize_grouped_trusted(t->db, L->h_pairs.p, offs.data(), qk.data(), ql.data(), nl, t->p, &r, L->bound_n, false, verd.data())) return rc;
  std::vector<kmcpg_window_summary> s(nl);
  summaries_of_records(t->db, r, s.data());
  kmcpg_result_free(&r);
  for (uint32_t j = 0; j < nl; j++) out->s[idx[j]] = s[j];
  return 0;
}

}  // namespace

int wait_summary_impl(kmcpg_ticket* t, SummaryPart* out) {
  int rc = 0;
  if (t->pieces.empty()) rc = finish_summary(t, out);
  else {
    *out = SummaryPart();
    for (size_t i = 0; i < t->pieces.size() && rc == 0; i++) {
      SummaryPart one;
      if (t->pieces[i]) {
        kmcpg_ticket* w = t->pieces[i];
        t->pieces[i] = nullptr;
        rc = wait_summary_impl(w, &one);
      } else one = std::move(t->piece_sum[i]);
      if (rc) break;
      out->qlen.insert(out->qlen.end(), one.qlen.begin(), one.qlen.end());
      out->qkmers.insert(out->qkmers.end(), one.qkmers.begin(), one.qkmers.end());
      out->s.insert(out->s.end(), one.s.begin(), one.s.end());
      out->count(one);
    }
  }
  drop_after(t, rc);
  return rc;
}

int submit_handle(kmcpg_db* db, const kmcpg_params* params, kmcpg_params* p) {
  KMCPG_NO_FILES_ONLY(db);
  if (db->opts.shard_count != 1)
    return kmcpg_fail(KMCPG_EINVAL, "kmcpg_submit/kmcpg_search_batch need the whole database: open it on one GPU or with kmcpg_open_devices; use kmcpg_query_device + kmcpg_finalize per shard");
  if (db->shards.empty() && db->opts.device < 0 && db->paged_passes == 0) return kmcpg_fail(KMCPG_EDEVICE, "metadata-only handle (device -1): no GPU work possible");
  *p = params ? *params : default_params();
  if (p->min_matched < 1) return kmcpg_fail(KMCPG_EINVAL, "min_matched must be >= 1");
  if (int rcs = specific_refuse_params(db, *p)) return rcs;
  if (int rcs = counting_refuse_params(db, *p)) return rcs;
  return set_refuse_params(db, *p);
}

}  // namespace kmcpg

using namespace kmcpg;

static int submit_checked(kmcpg_db* db, const HostBatch& b, const kmcpg_params* params, bool block, kmcpg_ticket** out) {
  if (!db || !out || (b.n && (!b.seqs || !b.offs))) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *out = nullptr;
  if ((b.seqs2 == nullptr) != (b.offs2 == nullptr)) return kmcpg_fail(KMCPG_EINVAL, "seqs2 and offs2 must be given together");
  kmcpg_params p;
  if (int rc = submit_handle(db, params, &p)) return rc;
  return submit_impl(db, b, p, false, block, out);
}

extern "C" int kmcpg_submit(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const uint8_t* seqs2, const uint64_t* offs2, uint32_t n_reads,
                            const kmcpg_params* params, kmcpg_ticket** out) {
  return submit_checked(db, HostBatch{seqs, offs, seqs2, offs2, n_reads}, params, false, out);
}

extern "C" int kmcpg_wait(kmcpg_ticket* t, kmcpg_result* out) {
  if (!t || !out) {
    if (t) drop_ticket(t);
    return kmcpg_fail(KMCPG_EINVAL, "null argument");
  }
  if (t->summary) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_wait: a ticket of kmcpg_submit_windows_summary is consumed by kmcpg_wait_summaries (the ticket is still valid)");
  if (t->stats) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_wait: a ticket of kmcpg_submit_stats is consumed by kmcpg_wait_stats (the ticket is still valid)");
  if (t->bins) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_wait: a ticket of kmcpg_submit_bins is consumed by kmcpg_wait_bins (the ticket is still valid)");
  return wait_impl(t, out, false);
}

// reads [lo, lo + cnt) of a batch as a batch of their own: offsets of a part start at its first read — a rebased copy in o1 / o2 (the
// sequences themselves are addressed in place)
static HostBatch sub_batch(const HostBatch& b, uint32_t lo, uint32_t cnt, std::vector<uint64_t>& o1, std::vector<uint64_t>& o2) {
  o1.resize((size_t)cnt + 1);
  for (uint32_t r = 0; r <= cnt; r++) o1[r] = b.offs[lo + r] - b.offs[lo];
  if (b.offs2) {
    o2.resize((size_t)cnt + 1);
    for (uint32_t r = 0; r <= cnt; r++) o2[r] = b.offs2[lo + r] - b.offs2[lo];
  }
  return HostBatch{b.seqs + b.offs[lo], o1.data(), b.seqs2 ? b.seqs2 + b.offs2[lo] : nullptr, b.offs2 ? o2.data() : nullptr, cnt};
}

// One large batch, several pieces in flight.  kmcpg_search_batch is a synchronous call: upload, K1 + K2 + K3, the copy of the ordered
// pairs and their expansion to Match records would follow each other with nothing overlapped (on a database of close relatives —
// 200 matches per read — the copy and the expansion take as long as the kernels).  Here the batch is cut into up to 4 pieces of at
// least 16 384 queries that go through the handle's lanes one behind the other: while the GPU works on piece j + 1, piece j comes
// down and is written straight into its place in the ONE result of the call (finalize_grouped_into), so the result is exactly that of
// the unsplit batch and nothing is copied twice.  Taken when the handle holds the whole database on one GPU with K3 on and no query can
// need a second search (may_retry: those splice sub-results and keep the plain path).
// A thread only ever BLOCKS for a lane while it holds none (two threads in here at once share the lanes instead of waiting for each
// other's).  *took = false: not applicable, nothing done.
static int search_batch_pieces(kmcpg_db* db, const HostBatch& b, const kmcpg_params& p, bool as_pairs, kmcpg_result* out, bool* took) {
  const uint32_t n = b.n;
  *took = false;
  uint32_t kMinPiece = 16384;
  if (const char* e = getenv("KMCPG_PIECE_MIN")) kMinPiece = (uint32_t)std::max(1, atoi(e));  // tests and tools/stress_async.py: pieces of small batches
  int want = 4;
  if (const char* e = getenv("KMCPG_PIECES")) want = atoi(e);
  if (want < 2 || (uint64_t)n < 2 * (uint64_t)kMinPiece) return 0;
  if (!db->shards.empty() || db->paged_passes > 0 || db->opts.device < 0 || db->opts.shard_count != 1) return 0;
  if (may_retry(db, p, b.seqs2 != nullptr)) return 0;
  AsyncState* A = nullptr;
  if (int rc = async_state(db, &A)) return rc;
  if (!A->device_finalize || A->hits_stay_on_device) return 0;
  // The first large batch of a handle goes through whole: it teaches the handle how many hits to expect per read (hits_hint), so that
  // the pieces of later batches get hit buffers and eager copies of the right size at once.  (Cold, every piece would overflow its
  // buffer and run twice, and four lanes would allocate their pinned buffers inside the call: kmcp-search on a 100 000-read file
  // spent 0.34 s instead of 0.14 s in here.)
  if (A->hits_hint.load() == 0) return 0;
  const uint32_t S = (uint32_t)std::min<uint64_t>((uint64_t)want, std::min<uint64_t>(A->max_lanes, n / kMinPiece));
  if (S < 2) return 0;
  *took = true;
  struct Piece {
    Lane* lane = nullptr;
    uint32_t lo = 0, cnt = 0;
  };
  std::vector<Piece> pc(S);
  for (uint32_t j = 0; j < S; j++) {
    pc[j].lo = (uint32_t)((uint64_t)n * j / S);
    pc[j].cnt = (uint32_t)((uint64_t)n * (j + 1) / S) - pc[j].lo;
  }
  ResultOwner* o = result_owner_take();
  result_owner_shape(o, n, as_pairs);
  uint64_t match_base = 0;
  uint32_t next_finish = 0, next_submit = 0;
  int rc = 0;
  std::vector<uint64_t> o1, o2;
  const bool timing = getenv("KMCPG_FIN_TIMING") != nullptr;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_begin = now();
  auto finish_one = [&]() -> int {  // the oldest piece in flight: wait, bring its pairs down, expand them into their place
    Piece& q = pc[next_finish];
    uint64_t n_hits = 0;
    const double ta = now();
    int r = collect(db, A, q.lane, p, &n_hits);
    const double tb = now();
    uint64_t kept = 0;
    if (r == 0)
      r = finalize_grouped_into(db, q.lane->h_pairs.p, q.lane->h_roffs.p, q.lane->h_qk.p, q.lane->h_ql.p, q.cnt, p, o, q.lo, match_base, &kept, true, q.lane->bound_n,
                                q.lane->spec ? q.lane->h_verd.p : nullptr);
    if (timing)
      fprintf(stderr, "piece %u: collect from %.2f to %.2f ms, expanded by %.2f ms (%llu hits, %llu kept)\n", next_finish, ta - t_begin, tb - t_begin, now() - t_begin,
              (unsigned long long)n_hits, (unsigned long long)kept);
    if (r) drain(A);
    release_lane(A, q.lane, false);
    q.lane = nullptr;
    next_finish++;
    match_base += kept;
    return r;
  };
  while (rc == 0 && next_submit < S) {
    Lane* L = acquire_lane(A, false, next_finish == next_submit);  // block only while holding no lane
    if (!L) {
      rc = finish_one();
      continue;
    }
    Piece& q = pc[next_submit];
    q.lane = L;
    rc = stage(L, sub_batch(b, q.lo, q.cnt, o1, o2), !b.seqs2);
    if (rc == 0) rc = enqueue(db, A, L, p, true);
    if (timing) fprintf(stderr, "piece %u: enqueued at %.2f ms\n", next_submit, now() - t_begin);
    if (rc) {  // this piece never got as far as a completion event: drain and give its lane back, the older ones below
      keeping_error([&] { drain(A); });
      release_lane(A, L, false);
      q.lane = nullptr;
    } else next_submit++;
  }
  while (rc == 0 && next_finish < next_submit) rc = finish_one();
  if (rc) {
    keeping_error([&] {
      drain(A);
      for (uint32_t j = next_finish; j < next_submit; j++)
        if (pc[j].lane) release_lane(A, pc[j].lane, false);
      result_owner_give(o);
    });
    return rc;
  }
  result_publish(o, n, p.k > 0 ? p.k : db->info.k, out);
  return 0;
}

// kmcpg_search_batch / kmcpg_search_batch_pairs: as_pairs = the paths that can collect compact pairs natively do so (the caller converts
// whatever comes back as records)
static int search_batch_impl(kmcpg_db* db, const HostBatch& in, const kmcpg_params* params, bool as_pairs, kmcpg_result* out) {
  memset(out, 0, sizeof *out);
  kmcpg_ticket* t = nullptr;
  int rc = 0;
  bool took = false;
  if (db && in.n && in.seqs && in.offs && (in.seqs2 == nullptr) == (in.offs2 == nullptr)) {
    const kmcpg_params pp = params ? *params : default_params();
    if (int rcs = set_refuse_params(db, pp)) return rcs;
    if (int rcs = specific_refuse_params(db, pp)) return rcs;
    if (int rcs = counting_refuse_params(db, pp)) return rcs;
    if (pp.min_matched >= 1 && in.offs[0] == 0 && (!in.offs2 || in.offs2[0] == 0)) rc = search_batch_pieces(db, in, pp, as_pairs, out, &took);
  }
  if (took && rc == 0) return 0;
  // the counting stages have counted the pieces that were enqueued before one of them failed, and the batch is searched again below: they
  // would hold those reads twice (their read-outs refuse until the stage's reset)
  if (took) counting_taint(db, counting_mask(db));
  if (took) memset(out, 0, sizeof *out);
  if (!took || rc == KMCPG_ENOMEM) {
    rc = submit_checked(db, in, params, true, &t);
    if (rc == 0) rc = wait_impl(t, out, as_pairs);
  }
  if (rc != KMCPG_ENOMEM || in.n < 2) return rc;
  // The batch's workspace (8-24 B per base next to the resident index) or its hit buffers did not fit: the two halves of the
  // batch one after the other, their results joined — a caller that sized its batches for an emptier GPU gets its answer
  // instead of an error (the reference has no such limit: it searches query by query).  The halves split again if they must.
  // (One half may have taken a path that collects records — retries, a paged pass — and the other pairs: concat_results.)
  const std::string why = kmcpg_err_ref();
  const uint32_t h = in.n / 2;
  kmcpg_result part[2];
  for (int i = 0; i < 2; i++) {
    std::vector<uint64_t> o1, o2;
    rc = search_batch_impl(db, sub_batch(in, i ? h : 0, i ? in.n - h : h, o1, o2), params, as_pairs, &part[i]);
    if (rc) {
      if (i) kmcpg_result_free(&part[0]);
      return rc;
    }
  }
  concat_results(db, part, 2, in.n, as_pairs, part[0].k, out);
  if (getenv("KMCPG_VERBOSE")) fprintf(stderr, "kmcpg_search_batch: %u queries searched as two halves (%s)\n", in.n, why.c_str());
  return 0;
}

extern "C" int kmcpg_search_batch(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const uint8_t* seqs2, const uint64_t* offs2, uint32_t n_reads,
                                  const kmcpg_params* params, kmcpg_result* out) {
  if (!out) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  return search_batch_impl(db, HostBatch{seqs, offs, seqs2, offs2, n_reads}, params, false, out);
}

// ---- compact results: the internal forms of search and wait are asked for pairs (results shaped on the way collect pairs, finalize.cpp), then
//      whatever a path without native pairs produced (retries, host-merged lists, paged passes) is converted.  Batches whose queries may be
//      searched again (may_retry) have their sub-results spliced record by record: they collect records and are converted at the end
namespace {
int publish_pairs(kmcpg_result* r, kmcpg_result_pairs* out) {
  ResultOwner* o = (ResultOwner*)r->owner;
  memset(out, 0, sizeof *out);
  if (!o) return 0;  // an empty result
  result_records_to_pairs(o);
  out->n_reads = r->n_reads;
  out->k = r->k;
  out->qlen = o->qlen.data();
  out->qkmers = o->qkmers.data();
  out->ksize = o->ksize.data();
  out->match_offs = o->offs.data();
  out->pairs = o->pairs.data();
  out->owner = o;
  memset(r, 0, sizeof *r);
  return 0;
}
}  // namespace

extern "C" int kmcpg_search_batch_pairs(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const uint8_t* seqs2, const uint64_t* offs2, uint32_t n_reads,
                                        const kmcpg_params* params, kmcpg_result_pairs* out) {
  if (!out) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  const bool native = db && !may_retry(db, params ? *params : default_params(), seqs2 != nullptr);
  kmcpg_result r{};
  if (int rc = search_batch_impl(db, HostBatch{seqs, offs, seqs2, offs2, n_reads}, params, native, &r)) return rc;
  return publish_pairs(&r, out);
}

extern "C" int kmcpg_wait_pairs(kmcpg_ticket* t, kmcpg_result_pairs* out) {
  if (!t || !out) {
    if (t) drop_ticket(t);
    return kmcpg_fail(KMCPG_EINVAL, "null argument");
  }
  if (t->summary) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_wait_pairs: a ticket of kmcpg_submit_windows_summary is consumed by kmcpg_wait_summaries (the ticket is still valid)");
  if (t->stats) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_wait_pairs: a ticket of kmcpg_submit_stats is consumed by kmcpg_wait_stats (the ticket is still valid)");
  if (t->bins) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_wait_pairs: a ticket of kmcpg_submit_bins is consumed by kmcpg_wait_bins (the ticket is still valid)");
  memset(out, 0, sizeof *out);
  const bool native = !may_retry(t->db, t->p, t->paired);
  kmcpg_result r{};
  if (int rc = wait_impl(t, &r, native)) return rc;
  return publish_pairs(&r, out);
}

// ---- statistics-only search: the batch goes through the counting stages and K10 (lane.cpp), and nothing of its matches comes to the host
//      but the pairs of the reads the stages LEFT
extern "C" int kmcpg_submit_stats(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const uint8_t* seqs2, const uint64_t* offs2, uint32_t n_reads,
                                  const kmcpg_params* params, kmcpg_ticket** out) {
  const HostBatch b{seqs, offs, seqs2, offs2, n_reads};
  if (!db || !out || (b.n && (!b.seqs || !b.offs))) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *out = nullptr;
  if ((b.seqs2 == nullptr) != (b.offs2 == nullptr)) return kmcpg_fail(KMCPG_EINVAL, "seqs2 and offs2 must be given together");
  if (!counting_mask(db)) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_submit_stats: no counting stage is on: call kmcpg_set_refstats, kmcpg_set_cooccur or kmcpg_set_recount first");
  if (db->spec_on())
    return kmcpg_fail(KMCPG_EINVAL, "kmcpg_submit_stats: the species-specific stage (kmcpg_set_specific) is on — it filters a result this ticket does not have; switch it off");
  if (int rc = set_refuse_entry(db, "kmcpg_submit_stats")) return rc;
  if (int rc = refuse_handle(db, "statistics-only searches (kmcpg_submit_stats)", "the counting stages need a query's matches from every block")) return rc;
  kmcpg_params p;
  if (int rc = submit_handle(db, params, &p)) return rc;
  AsyncState* A = nullptr;
  if (int rc = async_state(db, &A)) return rc;
  if (!A->device_finalize || A->hits_stay_on_device)
    return kmcpg_fail(KMCPG_EUNSUPPORTED, "kmcpg_submit_stats needs K3 on the device (KMCPG_DEVICE_FINALIZE=0 is set): use kmcpg_submit and kmcpg_wait");
  return submit_impl(db, b, p, false, false, out, nullptr, false, true);
}

extern "C" int kmcpg_wait_stats(kmcpg_ticket* t, kmcpg_result_stats* out) {
  if (!t || !out) {
    if (t) drop_ticket(t);
    return kmcpg_fail(KMCPG_EINVAL, "null argument");
  }
  if (!t->stats) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_wait_stats: the ticket is not one of kmcpg_submit_stats (it is still valid)");  // (one of kmcpg_submit_bins is none)
  memset(out, 0, sizeof *out);
  kmcpg_db* db = t->db;
  int rc = 0;
  kmcpg_stats_ticket_stats st{};
  st.k10_ms = -1;
  if (t->n) {
    auto& pt = t->parts[0];
    Lane* L = pt.lane;
    uint64_t n_hits = 0;
    rc = collect(pt.shard, pt.shard->async, L, t->p, &n_hits, false);
    if (rc == 0 && !L->stats_only()) rc = kmcpg_fail(KMCPG_EDEVICE, "internal: a statistics-only batch did not go through K10");
    if (rc == 0 && L->h_roffs.p[(size_t)t->n + 1] != 0)
      rc = kmcpg_fail(KMCPG_EINVAL, "%llu hit(s) named a read or column that does not exist", (unsigned long long)L->h_roffs.p[(size_t)t->n + 1]);
    if (rc == 0) st = L->left_res;
  }
  if (rc == 0) {
    out->n_reads = st.n_reads, out->matched_reads = st.matched_reads, out->kept_pairs = st.kept_pairs;
    out->left_reads = st.left_reads, out->left_pairs = st.left_pairs, out->bytes_d2h = st.bytes_d2h;
    std::lock_guard<std::mutex> g(db->mu);
    db->left_ticket = st;
    db->left_from_ticket = true;
    db->left_ran = true;
  }
  drop_after(t, rc);
  return rc;
}

// ---- binning search: the batch goes through K3 and K11 (lane.cpp), and nothing of its matches comes to the host but the pairs of the
//      reads K11 LEFT
extern "C" int kmcpg_submit_bins(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const uint8_t* seqs2, const uint64_t* offs2, uint32_t n_reads,
                                 const kmcpg_params* params, kmcpg_ticket** out) {
  const HostBatch b{seqs, offs, seqs2, offs2, n_reads};
  if (!db || !out || (b.n && (!b.seqs || !b.offs))) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *out = nullptr;
  if ((b.seqs2 == nullptr) != (b.offs2 == nullptr)) return kmcpg_fail(KMCPG_EINVAL, "seqs2 and offs2 must be given together");
  if (!db->binning_on()) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_submit_bins: the stage is off: call kmcpg_set_binning first");
  if (db->spec_on())
    return kmcpg_fail(KMCPG_EINVAL, "kmcpg_submit_bins: the species-specific stage (kmcpg_set_specific) is on — it filters a result this ticket does not have; switch it off");
  if (int rc = set_refuse_entry(db, "kmcpg_submit_bins")) return rc;
  if (int rc = refuse_handle(db, "binning searches (kmcpg_submit_bins)", "a query's bin needs its matches from every block")) return rc;
  kmcpg_params p;
  if (int rc = submit_handle(db, params, &p)) return rc;
  if (const char* what = final_matches_refused(db, p))
    return kmcpg_fail(KMCPG_EUNSUPPORTED, "taxonomic bins (kmcpg_set_binning): %s is not supported — bin the results with kmcp-refstats --binning", what);
  AsyncState* A = nullptr;
  if (int rc = async_state(db, &A)) return rc;
  if (!A->device_finalize || A->hits_stay_on_device)
    return kmcpg_fail(KMCPG_EUNSUPPORTED, "kmcpg_submit_bins needs K3 on the device (KMCPG_DEVICE_FINALIZE=0 is set): use kmcpg_submit and kmcpg_wait");
  return submit_impl(db, b, p, false, false, out, nullptr, false, false, true);
}

extern "C" int kmcpg_wait_bins(kmcpg_ticket* t, uint32_t* bins, kmcpg_result_bins* out) {
  if (!t || !out || (t->n && !bins)) {
    if (t) drop_ticket(t);
    return kmcpg_fail(KMCPG_EINVAL, "null argument");
  }
  if (!t->bins) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_wait_bins: the ticket is not one of kmcpg_submit_bins (it is still valid)");
  memset(out, 0, sizeof *out);
  kmcpg_db* db = t->db;
  int rc = 0;
  kmcpg_bin_stats st{};
  st.k11_ms = -1;
  if (t->n) {
    auto& pt = t->parts[0];
    Lane* L = pt.lane;
    uint64_t n_hits = 0;
    rc = collect(pt.shard, pt.shard->async, L, t->p, &n_hits, false);
    if (rc == 0 && !L->bins_only()) rc = kmcpg_fail(KMCPG_EDEVICE, "internal: a binning batch did not go through K11");
    if (rc == 0 && L->h_roffs.p[(size_t)t->n + 1] != 0)
      rc = kmcpg_fail(KMCPG_EINVAL, "%llu hit(s) named a read or column that does not exist", (unsigned long long)L->h_roffs.p[(size_t)t->n + 1]);
    if (rc == 0) {
      st = L->bin_res;
      memcpy(bins, L->h_bins.p, (size_t)t->n * sizeof(uint32_t));
      out->n_reads = t->n;
      out->kept_pairs = L->bin_kept_pairs, out->host_reads = st.left, out->left_pairs = L->bin_left_pairs, out->bytes_d2h = L->bin_bytes_d2h;
      out->reruns = L->reruns;
      for (uint32_t r = 0; r < t->n; r++) out->binned_reads += bins[r] != KMCPG_BIN_NONE;
    }
  }
  if (rc == 0) {
    std::lock_guard<std::mutex> g(db->mu);
    db->bin_ticket = st;
    db->bin_from_ticket = true;
    db->bin_ran = true;
  }
  drop_after(t, rc);
  return rc;
}

// How many bases a batch may hold on this handle so that its workspace fits beside the resident index: K1/K1d take up to 24 B
// per base (8 B of hashes, 16 B of sort scratch for queries above -u and for window sketches; query.cpp), the lanes another few
// bytes per base of staging.  A paged handle answers from the reserve plan_passes() kept free beside its largest shard, every
// other handle from the HBM free right now.  *max_bases = 0: unknown (the device would not say).
extern "C" int kmcpg_batch_hint(const kmcpg_db* db, uint64_t* max_bases) {
  if (!db || !max_bases) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  uint64_t room = 0;
  if (db->paged_passes > 1) room = db->paged_reserve;
  else if (db->opts.device >= 0) {
    int cur = -1;
    (void)hipGetDevice(&cur);
    size_t fr = 0, tot = 0;
    if (hipSetDevice(db->opts.device) == hipSuccess && hipMemGetInfo(&fr, &tot) == hipSuccess) room = fr;
    else (void)hipGetLastError();
    if (cur >= 0) (void)hipSetDevice(cur);
  }
  *max_bases = room / 40;  // 24 B/base of workspace + staging of the lanes in flight + headroom for the hit buffers
  return 0;
}
