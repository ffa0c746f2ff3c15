// host_windows.cpp — sliding windows of long queries above the lanes (kmcpg_submit_windows and its kin): a batch's windows are cut into
// pieces (window_plan.hpp), a piece is searched with its windows read in place on the device or cut into text on the host, and the pieces'
// results come back as one — as matches, or as one summary per window (kmcpg_submit_windows_summary, K5).  The geometry itself — counts, pieces, what a piece stages — is window_plan.hpp's.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "lane.hpp"
#include "window_plan.hpp"

namespace kmcpg {
namespace {

// window bases one piece may hold: what kmcpg_batch_hint says fits beside the index, at most 256 M (6 GB of k-mer workspace)
uint64_t window_budget(const kmcpg_db* db) {
  uint64_t b = 1ull << 28, hint = 0;
  if (kmcpg_batch_hint(db, &hint) == 0 && hint > 0) b = std::min(b, hint);
  static const bool test_hooks = getenv("KMCPG_TEST_HOOKS") && atoi(getenv("KMCPG_TEST_HOOKS")) == 1;
  if (test_hooks)  // the fake ENOMEM of query.cpp: tests cut a read's windows over several pieces this way
    if (const char* e = getenv("KMCPG_TEST_MAX_BASES")) b = std::min<uint64_t>(b, (uint64_t)std::max(1ll, atoll(e)));
  return std::max<uint64_t>(b, 1);
}

// device path: the slices of reads the piece's windows cover go up as they are (a batch of reads, packed by stage() where that pays); the
// windows are descriptors built on the device (windows.hip) and read in place by the k-mer kernels
int submit_window_piece_device(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const kmcpg_window_spec& s, const WinPiece& pc,
                               const kmcpg_params& p, bool summary, kmcpg_ticket** out) {
  static thread_local std::vector<uint8_t> text;
  static thread_local WinStaging ws;
  stage_windows(offs, s, pc, (uint64_t)(p.k > 0 ? p.k : db->info.k), &ws);
  text.clear();
  for (const WinStaging::Copy& c : ws.copies) text.insert(text.end(), seqs + c.at, seqs + c.at + c.len);
  const uint32_t ns = (uint32_t)(ws.soffs.size() - 1);
  std::unique_ptr<kmcpg_ticket> t(new kmcpg_ticket());
  t->db = db;
  t->n = (uint32_t)pc.n_win;
  t->p = p;
  t->summary = summary;
  AsyncState* A = nullptr;
  if (int rc = async_state(db, &A)) return rc;
  Lane* L = acquire_lane(A, false, false);
  if (!L) return fail_all_lanes_busy(A);
  t->parts.push_back({db, L, false});
  int rc = stage(L, HostBatch{text.data(), ws.soffs.data(), nullptr, nullptr, ns}, true);  // the slices go up ...
  if (rc == 0 && L->h_wmeta.ensure(3 * ((size_t)ns + 1))) rc = kmcpg_fail(KMCPG_ENOMEM, "hipHostMalloc failed");
  if (rc == 0) {
    memcpy(L->h_wmeta.p, ws.wpre.data(), ((size_t)ns + 1) * sizeof(uint64_t));
    memcpy(L->h_wmeta.p + ns + 1, ws.vpre.data(), ((size_t)ns + 1) * sizeof(uint64_t));
    memcpy(L->h_wmeta.p + 2 * ((size_t)ns + 1), ws.cpre.data(), ((size_t)ns + 1) * sizeof(uint64_t));
    L->win = true;  // ... and the windows over them are what is searched
    L->n = (uint32_t)pc.n_win;
    L->tb1 = pc.bases;
    L->maxlen = (uint32_t)ws.wmax;
    L->wstep = s.step;
    L->wwin = s.window;
    L->wchunks = ws.cpre.back();
    L->summary = summary;
    rc = enqueue(db, A, L, p);
  }
  if (rc) {
    keeping_error([&] { drop_ticket(t.release(), true); });
    return rc;
  }
  t->S[0] = L->h_seqs.p;
  t->O[0] = L->h_offs.p;
  *out = t.release();
  return 0;
}

// host path (paged and multi-device handles, multi-k databases without an explicit k): the windows cut into text, searched as reads
int submit_window_piece_text(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const kmcpg_window_spec& s, const WinPiece& pc,
                             const kmcpg_params& p, bool summary, kmcpg_ticket** out) {
  static thread_local std::vector<uint8_t> text;
  static thread_local std::vector<uint64_t> woffs;
  text.clear();
  woffs.assign(1, 0);
  for (const WinSlice& x : pc.sl) {
    const uint64_t L = offs[x.r + 1] - offs[x.r];
    for (uint64_t j = x.j0; j < x.j1; j++) {
      const uint64_t i = j * s.step, e = std::min<uint64_t>(i + s.window, L);
      text.insert(text.end(), seqs + offs[x.r] + i, seqs + offs[x.r] + e);
      woffs.push_back(text.size());
    }
  }
  return submit_impl(db, HostBatch{text.data(), woffs.data(), nullptr, nullptr, (uint32_t)pc.n_win}, p, false, false, out, nullptr, summary);
}

// summary: the ticket is one of kmcpg_submit_windows_summary (K5 behind K4, consumed by kmcpg_wait_summaries)
int submit_windows_impl(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, uint32_t n, const kmcpg_window_spec& s, const kmcpg_params& p,
                        kmcpg_ticket** out, bool summary = false) {
  // which handles read the windows in place: one GPU holding the whole index, and no search of the window text again (rereads_text: the
  // smaller k of a multi-k database).  KMCPG_WINDOWS_HOST=1 cuts text everywhere (A/B runs).
  static const bool host_env = getenv("KMCPG_WINDOWS_HOST") && atoi(getenv("KMCPG_WINDOWS_HOST")) == 1;
  const bool device = !host_env && db->paged_passes == 0 && db->shards.empty() && !rereads_text(db, p);
  const std::vector<WinPiece> pieces = plan_windows(offs, n, s, window_budget(db), 1ull << 22);
  auto one = [&](const WinPiece& pc, kmcpg_ticket** o) {
    return device ? submit_window_piece_device(db, seqs, offs, s, pc, p, summary, o) : submit_window_piece_text(db, seqs, offs, s, pc, p, summary, o);
  };
  if (pieces.empty()) {  // no read yields a window: an empty batch
    static const uint64_t zero = 0;
    return submit_impl(db, HostBatch{nullptr, &zero, nullptr, nullptr, 0}, p, false, false, out, nullptr, summary);
  }
  if (pieces.size() == 1) return one(pieces[0], out);
  uint64_t total = 0;
  for (const WinPiece& pc : pieces) total += pc.n_win;
  if (total > 0xffffffffULL) return kmcpg_fail(KMCPG_EUNSUPPORTED, "%llu windows in one batch: at most 2^32 - 1", (unsigned long long)total);
  std::unique_ptr<kmcpg_ticket> t(new kmcpg_ticket());
  t->db = db;
  t->n = (uint32_t)total;
  t->p = p;
  t->summary = summary;
  t->pieces.assign(pieces.size(), nullptr);
  t->piece_res.assign(pieces.size(), kmcpg_result{});
  if (summary) t->piece_sum.resize(pieces.size());
  size_t oldest = 0;  // pieces before this one are finished or waited for
  for (size_t i = 0; i < pieces.size(); i++) {
    for (;;) {
      int rc = one(pieces[i], &t->pieces[i]);
      if (rc == 0) break;
      // every lane in flight: finish this ticket's own oldest piece into its slot and take its lane (a caller whose other tickets hold every
      // lane gets KMCPG_EBUSY, as from kmcpg_submit)
      while (oldest < i && !t->pieces[oldest]) oldest++;
      if (rc == KMCPG_EBUSY && oldest < i) {
        kmcpg_ticket* w = t->pieces[oldest];
        t->pieces[oldest] = nullptr;
        rc = summary ? wait_summary_impl(w, &t->piece_sum[oldest]) : wait_impl(w, &t->piece_res[oldest], false);
      }
      if (rc) {
        keeping_error([&] { drop_ticket(t.release(), true); });
        return rc;
      }
    }
  }
  *out = t.release();
  return 0;
}

int window_args(const uint64_t* offs, uint32_t n_reads, const kmcpg_window_spec* spec) {
  if (n_reads && !offs) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (int rc = window_spec_args(spec)) return rc;
  uint64_t maxlen = 0;
  if (int rc = check_offsets(HostBatch{nullptr, offs, nullptr, nullptr, n_reads}, &maxlen)) return rc;
  if (maxlen > 0x7fffffffULL) return kmcpg_fail(KMCPG_EUNSUPPORTED, "query longer than 2^31-1 bases");
  return 0;
}

}  // namespace

int window_spec_args(const kmcpg_window_spec* spec) {
  if (!spec) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (spec->step < 1 || spec->window < 1) return kmcpg_fail(KMCPG_EINVAL, "window spec: step and window must be >= 1");
  // (a negative value from a caller that meant a signed type arrives as ~2^64: refused, as is anything in the fields the ABI keeps for later)
  if (spec->step > (1ull << 40) || spec->window > (1ull << 40)) return kmcpg_fail(KMCPG_EINVAL, "window spec: step and window must be <= 2^40");
  if (spec->greedy != 0 && spec->greedy != 1) return kmcpg_fail(KMCPG_EINVAL, "window spec: greedy must be 0 or 1");
  if (spec->reserved != 0) return kmcpg_fail(KMCPG_EINVAL, "window spec: reserved must be 0 (zero the struct)");
  return 0;
}

// a ticket of several window pieces: their results one behind the other, as one result (the record or the compact form the caller asked for)
int wait_pieces(kmcpg_ticket* t, kmcpg_result* out, bool as_pairs) {
  const size_t np = t->pieces.size();
  std::vector<kmcpg_result> rs(np);
  int rc = 0;
  for (size_t i = 0; i < np && rc == 0; i++) {
    if (t->pieces[i]) {
      kmcpg_ticket* w = t->pieces[i];
      t->pieces[i] = nullptr;
      rc = wait_impl(w, &rs[i], as_pairs);
    } else {
      rs[i] = t->piece_res[i];
      t->piece_res[i] = kmcpg_result{};
    }
  }
  if (rc) {
    for (kmcpg_result& r : rs) kmcpg_result_free(&r);
    return rc;
  }
  concat_results(t->db, rs.data(), np, t->n, as_pairs, t->p.k > 0 ? t->p.k : t->db->info.k, out);
  return 0;
}

}  // namespace kmcpg

using namespace kmcpg;

extern "C" int kmcpg_window_count(const uint64_t* offs, uint32_t n_reads, const kmcpg_window_spec* spec, uint64_t* n_windows, uint64_t* window_bases) {
  if (int rc = window_args(offs, n_reads, spec)) return rc;
  uint64_t nw = 0, nb = 0;
  for (uint32_t r = 0; r < n_reads; r++) {
    const uint64_t L = offs[r + 1] - offs[r], c = win_count(L, *spec);
    nw += c;
    nb += win_bases_before(L, c, *spec);
  }
  if (n_windows) *n_windows = nw;
  if (window_bases) *window_bases = nb;
  return 0;
}

extern "C" int kmcpg_window_locate(const uint64_t* offs, uint32_t n_reads, const kmcpg_window_spec* spec, uint64_t first, uint64_t n, uint32_t* read,
                                   uint64_t* start) {
  if (int rc = window_args(offs, n_reads, spec)) return rc;
  if (n && (!read || !start)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  uint64_t w = 0, done = 0;
  for (uint32_t r = 0; r < n_reads && done < n; r++) {
    const uint64_t c = win_count(offs[r + 1] - offs[r], *spec);
    for (uint64_t j = first > w ? first - w : 0; j < c && done < n; j++) {
      read[done] = r;
      start[done] = j * spec->step;
      done++;
    }
    w += c;
  }
  if (done < n) return kmcpg_fail(KMCPG_EINVAL, "rows %llu .. %llu: the batch has %llu windows", (unsigned long long)first, (unsigned long long)(first + n - 1), (unsigned long long)w);
  return 0;
}

extern "C" int kmcpg_submit_windows(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, uint32_t n_reads, const kmcpg_window_spec* spec,
                                    const kmcpg_params* params, kmcpg_ticket** out) {
  if (!db || !out || (n_reads && (!seqs || !offs))) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *out = nullptr;
  if (int rc = set_refuse_entry(db, "kmcpg_submit_windows")) return rc;
  if (int rc = specific_refuse_entry(db, "kmcpg_submit_windows")) return rc;
  if (int rc = counting_refuse_entry(db, "kmcpg_submit_windows")) return rc;
  kmcpg_params p;
  if (int rc = submit_handle(db, params, &p)) return rc;
  if (int rc = window_args(offs, n_reads, spec)) return rc;
  return submit_windows_impl(db, seqs, offs, n_reads, *spec, p, out);
}

extern "C" int kmcpg_submit_packed_windows(kmcpg_db* db, const uint8_t* codes, const uint64_t* offs, const kmcpg_exc_run* exc, uint64_t n_exc,
                                           uint32_t n_reads, const kmcpg_window_spec* spec, const kmcpg_params* params, kmcpg_ticket** out) {
  if (!db || !out || (n_reads && (!codes || !offs)) || (n_exc && !exc)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *out = nullptr;
  if (int rc = set_refuse_entry(db, "kmcpg_submit_packed_windows")) return rc;
  if (int rc = specific_refuse_entry(db, "kmcpg_submit_packed_windows")) return rc;
  if (int rc = counting_refuse_entry(db, "kmcpg_submit_packed_windows")) return rc;
  kmcpg_params p;
  if (int rc = submit_handle(db, params, &p)) return rc;
  if (int rc = window_args(offs, n_reads, spec)) return rc;
  // the reads' bases once as text on the host (not the windows'): the slices a piece needs are cut from it and go up packed again where that
  // pays (stage)
  std::vector<uint8_t> text;  // (released on return: the pieces have been staged by then)
  const uint64_t tb = n_reads ? offs[n_reads] : 0;
  text.resize(tb + 1);
  if (int rc = kmcpg_unpack2(codes, tb, exc, n_exc, text.data())) return rc;
  return submit_windows_impl(db, text.data(), offs, n_reads, *spec, p, out);
}

// ---- window summaries (K5 behind K4): the entry of kmcp-search --regions-bed
namespace {
struct SummaryOwner {
  SummaryPart part;
};
}  // namespace

extern "C" int kmcpg_submit_windows_summary(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, uint32_t n_reads, const kmcpg_window_spec* spec,
                                            const kmcpg_params* params, kmcpg_ticket** out) {
  if (!db || !out || (n_reads && (!seqs || !offs))) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *out = nullptr;
  if (int rc = set_refuse_entry(db, "kmcpg_submit_windows_summary")) return rc;
  if (int rc = counting_refuse_entry(db, "kmcpg_submit_windows_summary")) return rc;
  if (!db->spec_on()) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_submit_windows_summary: the species-specific stage is off: call kmcpg_set_specific first");
  kmcpg_params p;
  if (int rc = submit_handle(db, params, &p)) return rc;
  if (int rc = window_args(offs, n_reads, spec)) return rc;
  return submit_windows_impl(db, seqs, offs, n_reads, *spec, p, out, true);
}

extern "C" int kmcpg_wait_summaries(kmcpg_ticket* t, kmcpg_result_summaries* out) {
  if (!t || !out) {
    if (t) drop_ticket(t);
    return kmcpg_fail(KMCPG_EINVAL, "null argument");
  }
  if (t->stats) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_wait_summaries: a ticket of kmcpg_submit_stats is consumed by kmcpg_wait_stats (the ticket is still valid)");
  if (t->bins) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_wait_summaries: a ticket of kmcpg_submit_bins is consumed by kmcpg_wait_bins (the ticket is still valid)");
  if (!t->summary) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_wait_summaries: the ticket is not one of kmcpg_submit_windows_summary (it is still valid: kmcpg_wait / kmcpg_wait_pairs)");
  memset(out, 0, sizeof *out);
  kmcpg_db* db = t->db;
  std::unique_ptr<SummaryOwner> o(new SummaryOwner());
  if (int rc = wait_summary_impl(t, &o->part)) return rc;
  SummaryPart& s = o->part;
  kmcpg_summary_stats st{};
  st.single = s.single, st.wave = s.wave, st.left = s.left, st.empty = s.empty;
  st.left_pairs = s.left_pairs;
  st.bytes_d2h = s.bytes_d2h;
  {
    std::lock_guard<std::mutex> g(db->mu);
    db->sum_ticket = st;
    db->sum_from_ticket = true;
    db->sum_ran = true;
  }
  out->n_windows = (uint32_t)s.s.size();
  out->qlen = s.qlen.data();
  out->qkmers = s.qkmers.data();
  out->s = s.s.data();
  out->owner = o.release();
  return 0;
}

extern "C" void kmcpg_result_summaries_free(kmcpg_result_summaries* r) {
  if (!r) return;
  delete (SummaryOwner*)r->owner;
  memset(r, 0, sizeof *r);
}
