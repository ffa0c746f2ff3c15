// sketch.cpp — `kmcp compute` for a batch of joined reference genomes (kmcp/cmd/compute.go:675-826), without a database handle: the
// chunks of every genome (split_plan.hpp), their k-mer hashes by the K1 kernels of the search path (k1_plan.hpp decides the form; the
// chunks are views into the uploaded genomes, K1Args::src, as sliding windows are), and the sort + unique of all chunk lists of a
// piece in one set of launches (sort_segments.hip).  build.cpp takes the lists from there (kmcpg_build_col).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "sort_segments.hpp"
#include "split_plan.hpp"

using namespace kmcpg;

struct kmcpg_sketcher {
  std::mutex mu;
  kmcpg_sketch_cfg cfg{};
  int32_t device = 0;
  int mode = 0;  // 0 plain (+scaled), 1 minimizer, 2 syncmer
  uint32_t w_or_s = 0;
  uint64_t max_hash = ~0ULL;
  int key_bits = 64;
  hipStream_t st = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  DevBuf<uint8_t> d_text;
  DevBuf<uint64_t> d_src, d_offs, d_hashes, d_scratch, d_koff;
  DevBuf<int32_t> d_nk, d_nk1, d_qlen;
  DevBuf<uint32_t> d_side, d_temp;
  std::vector<kmcpg_sketch_launch> log;
  float kmers_ms = 0, sort_ms = 0;
};

namespace {

struct SketchOwner {
  std::vector<uint32_t> genome, chunk_idx, chunks;
  std::vector<uint64_t> koff;
  uint64_t* hashes = nullptr;
};

uint64_t sketch_max_hash(uint32_t scale) {
  // uint64(float64(^uint64(0)) / float64(scale))  (compute.go:309-311)
  const double d = 18446744073709551616.0 / (double)scale;
  if (d >= 18446744073709551616.0) return ~0ULL;
  return (uint64_t)d;
}

int check_spec(const kmcpg_split_spec* sp) {
  if (!sp) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (sp->reserved) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_split_spec.reserved must be 0");
  if (sp->split_number > 65535) return kmcpg_fail(KMCPG_EINVAL, "split_number should not be greater than 65535");  // compute.go:295
  if (sp->k_min < 1 || sp->k_max < sp->k_min) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_split_spec: 1 <= k_min <= k_max wanted");
  return 0;
}

SplitSpec to_plan(const kmcpg_split_spec& sp) {
  SplitSpec p;
  p.n = sp.split_number ? sp.split_number : 1;
  p.overlap = sp.split_overlap;
  p.min_ref = sp.split_min_ref;
  p.k_min = (uint64_t)sp.k_min;
  return p;
}

struct Chunk {
  uint64_t first, len;  // first base in the batch's text
  uint32_t genome, idx, of;
};

// the chunks of a call as a sink sees them, [all chunks]
struct ChunkMeta {
  std::vector<uint32_t> genome, chunk_idx, chunks;
};

// one piece: chunks [c0, c1) of the batch (text on the device already) -> sorted-unique lists on the device, handed to the sink
int sketch_piece(kmcpg_sketcher* s, const std::vector<Chunk>& ch, const ChunkMeta& meta, size_t c0, size_t c1, kmcpg_sketch_sink sink, void* user) {
  const uint32_t n = (uint32_t)(c1 - c0);
  const int nk = s->cfg.n_k;
  hipStream_t st = s->st;
  std::vector<uint64_t> h_src(n), h_offs(n + 1);
  uint64_t total = 0, max_len = 0, waves = 0;
  for (uint32_t i = 0; i < n; i++) {
    const Chunk& c = ch[c0 + i];
    h_src[i] = c.first;
    h_offs[i] = total;
    total += c.len;
    max_len = std::max(max_len, c.len);
    waves += seg_sort_waves_for(c.len * (uint64_t)nk);  // a chunk emits at most one hash per base and k-mer size
  }
  h_offs[n] = total;
  if (max_len > 0x7fffffffull / (uint64_t)nk) return kmcpg_fail(KMCPG_EUNSUPPORTED, "a chunk of %llu bases: at most 2^31 - 1 hashes per chunk", (unsigned long long)max_len);
  if (total * (uint64_t)nk >= (1ull << 32) || waves >= (1ull << 30))
    return kmcpg_fail(KMCPG_EUNSUPPORTED, "a piece of %llu bases x %d k-mer sizes: lower KMCPG_SKETCH_PIECE_BASES", (unsigned long long)total, nk);
  const uint64_t stride = total + 1;
  const size_t temp_words = seg_sort_temp_words(n, (uint32_t)waves);
  if (s->d_src.ensure(n + 1) || s->d_offs.ensure(n + 1) || s->d_hashes.ensure((size_t)nk * stride) || s->d_scratch.ensure((size_t)std::max(nk, 2) * stride) ||
      s->d_nk.ensure((size_t)nk * (n + 1)) || s->d_nk1.ensure(n + 1) || s->d_qlen.ensure(n + 1) || s->d_temp.ensure(temp_words) || s->d_koff.ensure(n + 2))
    return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed (a piece of %llu bases: lower KMCPG_SKETCH_PIECE_BASES)", (unsigned long long)total);
  HIPCHK(hipMemcpyAsync(s->d_src.p, h_src.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(s->d_offs.p, h_offs.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(s->ev[0], st));
  for (int j = 0; j < nk; j++) {
    K1Shape sh;
    sh.mode = s->mode;
    sh.k = s->cfg.ks[j];
    sh.w_or_s = s->w_or_s;
    sh.n_reads = n;
    sh.max_read_len = (uint32_t)max_len;
    sh.have_scratch = true;
    sh.dedup_threshold = 0x7fffffff;  // every emission stays in hashes[]: the segmented sort takes them all (as kmcpg_plant_reads_device asks)
    const K1Plan plan = k1_plan(sh);
    if (s->d_side.ensure(plan.side_words + 1)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed");
    uint32_t* const side = s->d_side.p;
    auto side_at = [side](const K1Region& r) { return r.len ? side + r.off : nullptr; };
    K1Args a{};
    a.seqs = s->d_text.p;
    a.offs = s->d_offs.p;
    a.n_reads = n;
    a.k = sh.k;
    a.min_qlen = 0;
    a.scaled = s->cfg.scale > 1;
    a.max_hash = s->max_hash;
    a.mode = s->mode;
    a.w_or_s = s->w_or_s;
    a.hashes = s->d_hashes.p + (size_t)j * stride;
    a.scratch = s->d_scratch.p;
    a.scratch2 = s->d_scratch.p + stride;
    a.nk_raw = s->d_nk.p + (size_t)j * (n + 1);
    a.nk1 = s->d_nk1.p;
    a.qlen = s->d_qlen.p;
    a.flags = sh.knobs.flags;
    a.seg_cnt = (int32_t*)side_at(plan.counts);
    a.segs_max = plan.segs;
    a.seg_nflag = side_at(plan.counter);
    a.seg_list = side_at(plan.list);
    a.seg_exc = side_at(plan.marks);
    a.seg_only_flagged = plan.list_fallback;
    a.nk_adj = nullptr;
    a.dedup_threshold = sh.dedup_threshold;
    a.src = s->d_src.p;
    launch_k1(a, plan, K1WinOnce{}, st, nullptr);
  }
  HIPCHK(hipEventRecord(s->ev[1], st));
  SegSortIn in{};
  in.keys = s->d_hashes.p;
  in.in_off = s->d_offs.p;
  in.cnt = s->d_nk.p;
  in.part_stride = stride;
  in.cnt_stride = n + 1;
  in.parts = nk;
  in.n_segs = n;
  kmcpg_sketch_launch rec{};
  uint64_t* d_out = nullptr;
  if (seg_sort_unique(in, s->d_hashes.p, s->d_scratch.p, (uint32_t)waves, s->key_bits, s->d_temp.p, temp_words, s->d_koff.p, &d_out, &rec, st) != 0)
    return kmcpg_fail(KMCPG_EDEVICE, "segmented sort of %u chunk lists failed", n);
  HIPCHK(hipEventRecord(s->ev[2], st));
  std::vector<uint64_t> koff(n + 2);
  HIPCHK(hipMemcpyAsync(koff.data(), s->d_koff.p, (n + 2) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float a_ms = 0, b_ms = 0;
  HIPCHK(hipEventElapsedTime(&a_ms, s->ev[0], s->ev[1]));
  HIPCHK(hipEventElapsedTime(&b_ms, s->ev[1], s->ev[2]));
  s->kmers_ms += a_ms;
  s->sort_ms += b_ms;
  rec.keys = koff[n + 1];
  s->log.push_back(rec);
  const uint64_t uniq = koff[n];
  if (uniq > koff[n + 1] || koff[n + 1] > total * (uint64_t)nk) return kmcpg_fail(KMCPG_EDEVICE, "segmented sort: inconsistent counts (internal error)");
  koff[n + 1] = 0;  // the sink's koff has n + 1 entries
  kmcpg_sketch_piece piece{};
  piece.first_chunk = (uint32_t)c0;
  piece.n_chunks = n;
  piece.genome = meta.genome.data() + c0;
  piece.chunk_idx = meta.chunk_idx.data() + c0;
  piece.chunks = meta.chunks.data() + c0;
  piece.koff = koff.data();
  piece.d_hashes = d_out;
  piece.stream = (void*)st;
  const int rc = sink(user, &piece);
  // whatever the sink enqueued has run before the next piece (or the next call) reuses the buffers
  const hipError_t e = hipStreamSynchronize(st);
  if (rc) return rc;
  HIPCHK(e);
  return 0;
}

// the sink of kmcpg_sketch_genomes: every piece's lists down into page-locked memory of their own
struct HostSink {
  std::vector<uint64_t>* koff_all;
  std::vector<uint64_t*> bufs;
  std::vector<uint64_t> buf_n;
};

int host_sink(void* user, const kmcpg_sketch_piece* p) {
  HostSink* hs = (HostSink*)user;
  const uint64_t uniq = p->koff[p->n_chunks];
  uint64_t* h = nullptr;
  if (kmcpg_host_alloc(std::max<uint64_t>(uniq, 1) * sizeof(uint64_t), (void**)&h) != 0) return KMCPG_ENOMEM;
  hs->bufs.push_back(h);
  hs->buf_n.push_back(uniq);
  if (uniq) HIPCHK(hipMemcpyAsync(h, p->d_hashes, uniq * sizeof(uint64_t), hipMemcpyDeviceToHost, (hipStream_t)p->stream));
  const uint64_t base = hs->koff_all->back();
  for (uint32_t i = 1; i <= p->n_chunks; i++) hs->koff_all->push_back(base + p->koff[i]);
  return 0;
}

// the piece loop of both entry points: the genomes cut into chunks and uploaded once, then piece by piece through the sink
int sketch_run(kmcpg_sketcher* s, const uint8_t* seqs, const uint64_t* offs, uint32_t n_genomes, const kmcpg_split_spec* spec, kmcpg_sketch_sink sink,
               void* user, ChunkMeta* meta) {
  const int k_min = *std::min_element(s->cfg.ks, s->cfg.ks + s->cfg.n_k), k_max = *std::max_element(s->cfg.ks, s->cfg.ks + s->cfg.n_k);
  if (spec->k_min != k_min || spec->k_max != k_max) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_split_spec: k_min / k_max are not those of the sketcher (%d / %d)", k_min, k_max);
  HIPCHK(hipSetDevice(s->device));
  s->log.clear();
  s->kmers_ms = s->sort_ms = 0;
  const SplitSpec plan = to_plan(*spec);
  std::vector<Chunk> ch;
  std::vector<uint64_t> first, end;
  for (uint32_t gi = 0; gi < n_genomes; gi++) {
    if (offs[gi + 1] < offs[gi]) return kmcpg_fail(KMCPG_EINVAL, "offs must not decrease");
    const uint64_t len = offs[gi + 1] - offs[gi];
    const uint64_t cnt = split_bounds(len, plan, nullptr, nullptr, 0);
    first.resize(cnt);
    end.resize(cnt);
    split_bounds(len, plan, first.data(), end.data(), cnt);
    for (uint64_t c = 0; c < cnt; c++) ch.push_back(Chunk{offs[gi] + first[c], end[c] - first[c], gi, (uint32_t)c, (uint32_t)cnt});
  }
  for (const Chunk& c : ch) {
    meta->genome.push_back(c.genome);
    meta->chunk_idx.push_back(c.idx);
    meta->chunks.push_back(c.of);
  }
  if (ch.empty()) return 0;
  // every genome's bases go up once; the k-mer kernels may read a few bytes past a chunk's end (their staging): zeros behind the text
  const uint64_t text = offs[n_genomes] - offs[0], pad = 4096;
  if (s->d_text.ensure(text + pad)) return kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed (%llu bases of genomes)", (unsigned long long)text);
  if (hipMemcpyAsync(s->d_text.p, seqs + offs[0], text, hipMemcpyHostToDevice, s->st) != hipSuccess ||
      hipMemsetAsync(s->d_text.p + text, 0, pad, s->st) != hipSuccess)
    return kmcpg_fail(KMCPG_EDEVICE, "upload of the genomes failed");
  for (Chunk& c : ch) c.first -= offs[0];
  uint64_t piece_max = 1ull << 28;
  if (const char* e = getenv("KMCPG_SKETCH_PIECE_BASES")) piece_max = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
  piece_max = std::min<uint64_t>(piece_max, ((1ull << 32) - 1) / (uint64_t)s->cfg.n_k - 1);
  size_t c0 = 0;
  while (c0 < ch.size()) {
    size_t c1 = c0;
    uint64_t bases = 0;
    while (c1 < ch.size() && (c1 == c0 || bases + ch[c1].len <= piece_max)) bases += ch[c1++].len;
    if (int rc = sketch_piece(s, ch, *meta, c0, c1, sink, user)) {
      (void)hipStreamSynchronize(s->st);  // the text upload of a call that ends early must not outlive the caller's buffer
      return rc;
    }
    c0 = c1;
  }
  return 0;
}

}  // namespace

extern "C" int kmcpg_sketcher_open(const kmcpg_sketch_cfg* cfg, int32_t device, kmcpg_sketcher** out) {
  if (!cfg || !out) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *out = nullptr;
  for (uint32_t r : cfg->reserved)
    if (r) return kmcpg_fail(KMCPG_EINVAL, "kmcpg_sketch_cfg.reserved must be 0");
  if (cfg->n_k < 1 || cfg->n_k > 8) return kmcpg_fail(KMCPG_EINVAL, "flag -k/--kmer needed: 1 to 8 k-mer sizes");
  for (int j = 0; j < cfg->n_k; j++) {
    if (cfg->ks[j] < 1) return kmcpg_fail(KMCPG_EINVAL, "invalid k: %d", cfg->ks[j]);                           // compute.go:177
    if (cfg->ks[j] > 64) return kmcpg_fail(KMCPG_EINVAL, "k-mer size (%d) should be <=64", cfg->ks[j]);          // :180
  }
  const int k_min = *std::min_element(cfg->ks, cfg->ks + cfg->n_k);
  if (cfg->minimizer_w && cfg->syncmer_s) return kmcpg_fail(KMCPG_EINVAL, "flag --minimizer-w and --syncmer-s can not be given simultaneously");  // :331
  if (cfg->syncmer_s >= (uint32_t)k_min && cfg->syncmer_s) return kmcpg_fail(KMCPG_EINVAL, "value of flag --syncmer-s should be smaller than k");
  if (cfg->minimizer_w > 1u << 20) return kmcpg_fail(KMCPG_EINVAL, "value of flag --minimizer-w is too big");
  if (device < 0) return kmcpg_fail(KMCPG_EDEVICE, "a sketcher needs a GPU (device >= 0)");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return kmcpg_fail(KMCPG_EDEVICE, "no HIP device");
  if (device >= n_dev) return kmcpg_fail(KMCPG_EDEVICE, "no HIP device %d (%d present)", device, n_dev);
  HIPCHK(hipSetDevice(device));
  kmcpg_sketcher* s = new kmcpg_sketcher();
  s->cfg = *cfg;
  s->device = device;
  s->mode = cfg->syncmer_s ? 2 : (cfg->minimizer_w ? 1 : 0);
  s->w_or_s = cfg->syncmer_s ? cfg->syncmer_s : cfg->minimizer_w;
  if (cfg->scale > 1) {
    s->max_hash = sketch_max_hash(cfg->scale);
    s->key_bits = s->max_hash ? 64 - __builtin_clzll(s->max_hash) : 1;
  }
  if (hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) != hipSuccess) {
    delete s;
    return kmcpg_fail(KMCPG_EDEVICE, "hipStreamCreate failed");
  }
  for (auto& e : s->ev)
    if (hipEventCreate(&e) != hipSuccess) {
      kmcpg_sketcher_close(s);
      return kmcpg_fail(KMCPG_EDEVICE, "hipEventCreate failed");
    }
  *out = s;
  return 0;
}

extern "C" int kmcpg_sketcher_close(kmcpg_sketcher* s) {
  if (!s) return 0;
  (void)hipSetDevice(s->device);
  if (s->st) (void)hipStreamSynchronize(s->st);
  s->d_text.release();
  s->d_src.release();
  s->d_offs.release();
  s->d_hashes.release();
  s->d_scratch.release();
  s->d_koff.release();
  s->d_nk.release();
  s->d_nk1.release();
  s->d_qlen.release();
  s->d_side.release();
  s->d_temp.release();
  for (auto& e : s->ev)
    if (e) (void)hipEventDestroy(e);
  if (s->st) (void)hipStreamDestroy(s->st);
  delete s;
  return 0;
}

extern "C" int kmcpg_split_bounds(uint64_t len, const kmcpg_split_spec* spec, uint64_t* first, uint64_t* end, uint64_t cap, uint64_t* n) {
  if (int rc = check_spec(spec)) return rc;
  if (!n || (cap && (!first || !end))) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  *n = split_bounds(len, to_plan(*spec), first, end, cap);
  return 0;
}

extern "C" void kmcpg_sketch_result_free(kmcpg_sketch_result* r) {
  if (!r) return;
  if (SketchOwner* o = (SketchOwner*)r->owner) {
    if (o->hashes) (void)kmcpg_host_free(o->hashes);
    delete o;
  }
  memset(r, 0, sizeof *r);
}

extern "C" int kmcpg_sketch_genomes(kmcpg_sketcher* s, const uint8_t* seqs, const uint64_t* offs, uint32_t n_genomes, const kmcpg_split_spec* spec,
                                    kmcpg_sketch_result* out) {
  if (!s || !out || (n_genomes && (!seqs || !offs))) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (int rc = check_spec(spec)) return rc;
  memset(out, 0, sizeof *out);
  std::lock_guard<std::mutex> g(s->mu);
  SketchOwner* o = new SketchOwner();
  o->koff.push_back(0);
  HostSink hs;
  hs.koff_all = &o->koff;
  ChunkMeta meta;
  auto fail = [&](int rc) {
    for (uint64_t* b : hs.bufs) (void)kmcpg_host_free(b);
    delete o;
    return rc;
  };
  if (int rc = sketch_run(s, seqs, offs, n_genomes, spec, host_sink, &hs, &meta)) return fail(rc);
  // one contiguous list buffer: the only piece's, or the pieces' copied together
  if (hs.bufs.size() == 1) {
    o->hashes = hs.bufs[0];
  } else {
    const uint64_t all = o->koff.back();
    if (kmcpg_host_alloc(std::max<uint64_t>(all, 1) * sizeof(uint64_t), (void**)&o->hashes) != 0) return fail(KMCPG_ENOMEM);
    uint64_t at = 0;
    for (size_t i = 0; i < hs.bufs.size(); i++) {
      memcpy(o->hashes + at, hs.bufs[i], hs.buf_n[i] * sizeof(uint64_t));
      at += hs.buf_n[i];
      (void)kmcpg_host_free(hs.bufs[i]);
    }
  }
  o->genome = std::move(meta.genome);
  o->chunk_idx = std::move(meta.chunk_idx);
  o->chunks = std::move(meta.chunks);
  out->n_chunks = (uint32_t)o->genome.size();
  out->genome = o->genome.data();
  out->chunk_idx = o->chunk_idx.data();
  out->chunks = o->chunks.data();
  out->koff = o->koff.data();
  out->hashes = o->hashes;
  out->owner = o;
  return 0;
}

extern "C" int kmcpg_sketch_genomes_to(kmcpg_sketcher* s, const uint8_t* seqs, const uint64_t* offs, uint32_t n_genomes, const kmcpg_split_spec* spec,
                                       kmcpg_sketch_sink sink, void* user) {
  if (!s || !sink || (n_genomes && (!seqs || !offs))) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (int rc = check_spec(spec)) return rc;
  std::lock_guard<std::mutex> g(s->mu);
  ChunkMeta meta;
  return sketch_run(s, seqs, offs, n_genomes, spec, sink, user, &meta);
}

extern "C" int kmcpg_last_sketch_launches(kmcpg_sketcher* s, kmcpg_sketch_launch* out, uint32_t cap, uint32_t* n) {
  static_assert(sizeof(kmcpg_sketch_launch) == 32, "six 4-byte words and one of 8");
  if (!s || !n || (cap && !out)) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(s->mu);
  const size_t m = std::min<size_t>(cap, s->log.size());
  if (m) memcpy(out, s->log.data(), m * sizeof(kmcpg_sketch_launch));
  *n = (uint32_t)s->log.size();
  return 0;
}

extern "C" int kmcpg_last_sketch_ms(kmcpg_sketcher* s, float* kmers_ms, float* sort_ms) {
  if (!s) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(s->mu);
  if (kmers_ms) *kmers_ms = s->kmers_ms;
  if (sort_ms) *sort_ms = s->sort_ms;
  return 0;
}

// The segmented sort + unique on lists the caller laid out (tests): the buffers are arranged as sketch_piece arranges them — the raw
// lists in the sort's buffer a, a second buffer b of the same size — so that the radix passes alternate over the raw lists themselves.
extern "C" int kmcpg_sort_segments_device(const uint64_t* d_keys, const uint64_t* d_in_off, const int32_t* d_cnt, uint64_t part_stride,
                                          uint32_t cnt_stride, int32_t parts, uint32_t n_segs, uint32_t max_waves, int32_t key_bits,
                                          uint64_t* d_out, uint64_t out_cap, uint64_t* d_koff, kmcpg_sketch_launch* rec, void* stream) {
  if (!d_keys || !d_in_off || !d_cnt || !d_out || !d_koff) return kmcpg_fail(KMCPG_EINVAL, "null argument");
  if (parts < 1 || parts > 8) return kmcpg_fail(KMCPG_EINVAL, "parts = %d: 1 to 8 wanted", parts);
  if (key_bits < 0 || key_bits > 64) return kmcpg_fail(KMCPG_EINVAL, "key_bits = %d: 0 to 64 wanted", key_bits);
  if (cnt_stride < n_segs) return kmcpg_fail(KMCPG_EINVAL, "cnt_stride %u below n_segs %u", cnt_stride, n_segs);
  if (part_stride >= (1ull << 32) || max_waves >= (1u << 30)) return kmcpg_fail(KMCPG_EINVAL, "fewer than 2^32 raw keys and 2^30 waves wanted");
  const uint64_t words = part_stride * (uint64_t)parts;
  if (out_cap < words) return kmcpg_fail(KMCPG_EINVAL, "out_cap %llu below part_stride * parts = %llu", (unsigned long long)out_cap, (unsigned long long)words);
  hipStream_t st = (hipStream_t)stream;
  // the sizes come back to the host first: a list outside its part or more waves than max_waves would send the kernels out of bounds
  std::vector<int32_t> cnt((size_t)parts * n_segs);  // [parts][n_segs]
  std::vector<uint64_t> off(n_segs);
  if (n_segs) {
    for (int p = 0; p < parts; p++)
      HIPCHK(hipMemcpyAsync(cnt.data() + (size_t)p * n_segs, d_cnt + (size_t)p * cnt_stride, n_segs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(off.data(), d_in_off, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  uint64_t total = 0, waves = 0;
  for (uint32_t s = 0; s < n_segs; s++) {
    uint64_t n = 0;
    for (int p = 0; p < parts; p++) {
      const int32_t c = cnt[(size_t)p * n_segs + s];
      if (c < 0 || off[s] > part_stride || (uint64_t)c > part_stride - off[s])
        return kmcpg_fail(KMCPG_EINVAL, "segment %u, part %d: %d keys at in_off %llu do not fit part_stride %llu", s, p, c, (unsigned long long)off[s],
                          (unsigned long long)part_stride);
      n += (uint64_t)c;
    }
    total += n;
    waves += seg_sort_waves_for(n);
  }
  if (total >= (1ull << 32)) return kmcpg_fail(KMCPG_EINVAL, "%llu raw keys: fewer than 2^32 wanted", (unsigned long long)total);
  if (total > words)  // lists that overlap: the compact buffers hold part_stride * parts keys
    return kmcpg_fail(KMCPG_EINVAL, "%llu raw keys in part_stride * parts = %llu words: the lists overlap", (unsigned long long)total, (unsigned long long)words);
  if (waves > max_waves) return kmcpg_fail(KMCPG_EINVAL, "max_waves %u below the %llu waves of the segments", max_waves, (unsigned long long)waves);
  const size_t temp_words = seg_sort_temp_words(n_segs, max_waves);
  uint64_t *a = nullptr, *b = nullptr;
  uint32_t* temp = nullptr;
  auto done = [&](int rc) {
    (void)hipStreamSynchronize(st);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (temp) (void)hipFree(temp);
    return rc;
  };
  const size_t buf_bytes = (size_t)std::max<uint64_t>(words, 1) * sizeof(uint64_t);
  if (hipMalloc((void**)&a, buf_bytes) != hipSuccess || hipMalloc((void**)&b, buf_bytes) != hipSuccess ||
      hipMalloc((void**)&temp, temp_words * sizeof(uint32_t)) != hipSuccess)
    return done(kmcpg_fail(KMCPG_ENOMEM, "hipMalloc failed (%zu bytes of sort buffers)", 2 * buf_bytes + temp_words * sizeof(uint32_t)));
  if (words && hipMemcpyAsync(a, d_keys, words * sizeof(uint64_t), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return done(kmcpg_fail(KMCPG_EDEVICE, "copy of the raw lists failed"));
  SegSortIn in{};
  in.keys = a;
  in.in_off = d_in_off;
  in.cnt = d_cnt;
  in.part_stride = part_stride;
  in.cnt_stride = cnt_stride;
  in.parts = parts;
  in.n_segs = n_segs;
  kmcpg_sketch_launch r{};
  uint64_t* sorted = nullptr;
  if (seg_sort_unique(in, a, b, max_waves, key_bits, temp, temp_words, d_koff, &sorted, &r, st) != 0) {
    // of what the launcher refuses before it enqueues anything, only a key width without passes is left after the checks above
    if (max_waves && !seg_sort_passes(key_bits)) return done(kmcpg_fail(KMCPG_EINVAL, "key_bits = %d sorts no key: max_waves must be 0", key_bits));
    return done(kmcpg_fail(KMCPG_EDEVICE, "segmented sort of %u lists failed", n_segs));
  }
  uint64_t tail[2] = {0, 0};  // unique keys, raw keys
  if (hipMemcpyAsync(tail, d_koff + n_segs, sizeof tail, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return done(kmcpg_fail(KMCPG_EDEVICE, "segmented sort of %u lists failed on the device: %s", n_segs, hipGetErrorString(hipGetLastError())));
  if (tail[0] > tail[1] || tail[1] != total) return done(kmcpg_fail(KMCPG_EDEVICE, "segmented sort: inconsistent counts (internal error)"));
  if (tail[0] && hipMemcpyAsync(d_out, sorted, tail[0] * sizeof(uint64_t), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return done(kmcpg_fail(KMCPG_EDEVICE, "copy of the sorted lists failed"));
  r.keys = tail[1];
  if (rec) *rec = r;
  return done(hipStreamSynchronize(st) == hipSuccess ? 0 : kmcpg_fail(KMCPG_EDEVICE, "stream synchronisation failed"));
}
