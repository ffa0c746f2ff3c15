/*
 * kmcp_gpu.h — C ABI of libkmcpgpu.so: the MI355X-native replacement of the `kmcp search` hot path.
 *
 * The reference (shenwei356/kmcp v0.9.5, pure Go) has no FFI seam; the seam is a pair of Go channel
 * protocols inside package cmd.  Each entry point below names the reference code it
 * replaces (paths relative to kmcp/cmd/).  The cgo binding a maintainer would add is shim/kmcp_gpu.go
 * (see INTEGRATION.md).
 *
 * Conventions: every function returns 0 on success or a negative KMCPG_E* code; the message is
 * available from kmcpg_last_error() (thread-local).  No exception or abort crosses the ABI.  Input
 * buffers are borrowed for the duration of the call only; buffers returned inside kmcpg_result are
 * owned by the library and released by kmcpg_result_free().  A kmcpg_db may be used from several OS
 * threads: the enqueueing of GPU work on one handle is serialised internally, and consecutive kmcpg_query_device calls
 * on different streams are ordered by an event (they share the handle's k-mer workspace), so they never overlap on the GPU.
 */
#ifndef KMCP_GPU_H
#define KMCP_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMCPG_OK 0
#define KMCPG_EINVAL (-1)   /* bad argument */
#define KMCPG_EIO (-2)      /* file missing / unreadable */
#define KMCPG_EFORMAT (-3)  /* invalid or incompatible .uniki / __db.yml (serialization.go:41-57) */
#define KMCPG_EDEVICE (-4)  /* HIP error, no GPU */
#define KMCPG_ENOMEM (-5)
#define KMCPG_EUNSUPPORTED (-6)
#define KMCPG_EBUSY (-7)    /* kmcpg_submit: every lane of the handle is in flight */

typedef struct kmcpg_db kmcpg_db;

/* How the database is placed on the GPU(s).  One process drives one GPU (one rank); the index's
 * independent .uniki blocks are partitioned over `shard_count` ranks by bytes. */
typedef struct {
  int32_t device;      /* HIP device ordinal of this process; -1 = metadata only (headers parsed, nothing resident:
                          kmcpg_db_info/col_info/block_info/finalize work, every GPU entry point fails) */
  int32_t shard_rank;  /* 0..shard_count-1 */
  int32_t shard_count; /* >=1 */
  int32_t reserved;
} kmcpg_opts;

/* What `search` needs to know about the database: UnikIndexDBInfo (util-db-info.go:46-79) + Header
 * (index/serialization.go:66-82). */
typedef struct {
  int32_t k;
  int32_t canonical;
  int32_t num_hashes;
  int32_t scaled;
  uint32_t scale;
  int32_t minimizer;
  uint32_t minimizer_w;
  int32_t syncmer;
  uint32_t syncmer_s;
  double fpr;             /* DB-wide false-positive rate of one Bloom filter (`fpr` in __db.yml) */
  int32_t n_blocks;       /* all .uniki files of the DB */
  int32_t n_blocks_local; /* blocks resident on this rank's GPU */
  uint64_t n_cols;        /* reference chunks (columns) over all blocks */
  uint64_t matrix_bytes;       /* on-disk bit-matrix bytes over all blocks */
  uint64_t matrix_bytes_local; /* on-disk bit-matrix bytes of the local blocks */
  uint64_t row_bytes_sum_local; /* sum over local blocks of NumRowBytes: algorithmic bytes per (k-mer, hash) */
} kmcpg_info;

/* SearchOptions (util-db-search.go:162-189); defaults are those of search.go:1052-1102. */
typedef struct {
  int32_t min_qlen;        /* -m/--min-query-len 30 */
  int32_t min_matched;     /* -c/--min-kmers 10 */
  double min_qcov;         /* -t/--min-query-cov 0.55 */
  double min_tcov;         /* -T/--min-target-cov 0 */
  double max_fpr;          /* -f/--max-fpr 0.01 */
  int32_t dedup_threshold; /* -u/--kmer-dedup-threshold 256 */
  int32_t try_se;          /* --try-se */
  int32_t sort_by;         /* -s: 0 qcov, 1 tcov, 2 jacc */
  int32_t do_not_sort;     /* -S */
  int32_t top_n_scores;    /* -n/--keep-top-scores */
  int32_t fpr_buf_size;    /* 249 single-end / 499 paired-end (search.go:250-255); 0 = pick */
  int32_t k;               /* 0 = the database's k-mer sizes, largest first, smaller ones for queries that matched nothing
                              (util-db-search.go:764, :1016-1022); > 0 = this size only (must be one of the database's) */
  int32_t reserved;
} kmcpg_params;

/* One (read, reference chunk) pair that passed the integer thresholds on the GPU:
 * count >= max(min_matched, smallest c with float64(c) > n*min_qcov)   (util-db-search.go:7468-7470),
 * and, for queries of up to 1024 k-mers, count >= the smallest c whose FPR(n, c) <= max_fpr (:7474-7478): a pair that
 * kmcpg_finalize would drop for its FPR anyway is not reported (KMCPG_FPR_BOUND=0 reports it). */
typedef struct {
  uint32_t read;  /* index of the read in the batch */
  uint32_t col;   /* global column: columns numbered over the blocks in __db.yml `files` order */
  uint32_t count; /* matched k-mers (mKmers) */
} kmcpg_hit;

/* Match (util-db-search.go:83-93) without the strings; names come from kmcpg_col_info(). */
typedef struct {
  uint32_t col;
  uint32_t target_idx; /* chunkIdx | chunks<<16 (index.go:1096) */
  uint64_t gsize;
  int32_t mkmers;
  int32_t reserved;
  double fpr, qcov, tcov, jacc;
} kmcpg_match;

/* QueryResult (util-db-search.go:60-74) for a batch, CSR over reads. */
typedef struct {
  uint32_t n_reads;
  int32_t k;
  int32_t* qlen;         /* [n_reads] QueryLen (read1+read2 for paired-end; the searched mate after --try-se) */
  int32_t* qkmers;       /* [n_reads] NumKmers (0 when the query was not searched) */
  int32_t* ksize;        /* [n_reads] QueryResult.K: the k-mer size the query was last searched with (differs from `k` only in
                            databases with several k-mer sizes) */
  uint64_t* match_offs;  /* [n_reads+1] */
  kmcpg_match* matches;  /* [match_offs[n_reads]] sorted as handleQuerySingleDB does (:273-282) */
  void* owner;           /* internal */
} kmcpg_result;

/* -- lifecycle: replaces NewUnikIndexDB / NewUnikIndex (util-db-search.go:648-743, 1196-1280) and
 *    UnikIndexDB.Close (:1119-1150).  db_dir is the directory holding __db.yml (e.g. <db>/R001). */
int kmcpg_open(const char* db_dir, const kmcpg_opts* opts, kmcpg_db** out);
/* -- database sets: several databases searched in one pass, merged as `kmcp-merge` merges their separate results (the reference's profiling
 *    workflow: the same reads against GTDB, viral, fungi, then `kmcp merge`, kmcp/cmd/merge.go:40-420).  The members are opened as ONE handle on
 *    ONE GPU: the blocks of member m follow those of member m - 1, global columns are numbered over all of them (kmcpg_col_info /
 *    kmcpg_block_info work over the union), every member is resident (KMCPG_ENOMEM with the bytes needed / free, as kmcpg_open, when the
 *    sum does not fit).  opts->device == -1 opens metadata only.  1 to 16 members; with one member the handle IS a kmcpg_open handle.
 *    Contract: the result of every query is, byte for byte once printed, what kmcp-merge -s <sort_by> makes of the members' separate
 *    kmcp-search results — rows ordered by the PRINTED score (%.4f of qCov / tCov / jacc) descending, equal printed scores by member
 *    (argument order), then in the member's own row order; match_offs[i + 1] - match_offs[i] is the merged `hits`.
 *    The members must agree in everything a query's k-mers and thresholds depend on — one k-mer size each and the same one, canonical,
 *    scale, minimizer_w, syncmer_s, numHashes, fpr (the k-mer kernels run once per batch, a query has one NumKmers, the -f bound on the device
 *    is one table): KMCPG_EUNSUPPORTED names the field and the two directories.  Databases that disagree are searched one by one and merged
 *    with kmcp-merge.
 *    Refused on a set of two members or more (KMCPG_EUNSUPPORTED; each acts per member in separate runs and would act per query on the
 *    union): params try_se, do_not_sort, top_n_scores != 0, k != 0; kmcpg_save_db, kmcpg_submit_windows, kmcpg_submit_packed_windows,
 *    kmcpg_submit_packed; shard_count > 1.  There is no set form of kmcpg_open_paged / kmcpg_open_devices.  Everything else — kmcpg_submit,
 *    kmcpg_wait[_pairs], kmcpg_search_batch[_pairs], kmcpg_expand_pairs, paired-end input, lanes and tickets, kmcpg_query_device +
 *    kmcpg_group_device + kmcpg_finalize[_grouped] — works as on any other handle. */
int kmcpg_open_set(const char* const* db_dirs, uint32_t n, const kmcpg_opts* opts, kmcpg_db** out);
/* *n_members = members of the handle (1 for kmcpg_open handles, 0 for synthetic / files-only ones); the first global column of the first
 * min(*n_members, cap) members is written to first_col */
int kmcpg_set_info(const kmcpg_db* db, uint32_t* n_members, uint32_t* first_col, uint32_t cap);
/* What put the segments (the matches of one query) of a set handle into the merge order.  The device words are those of the handle's LAST
 * K3 launch (kmcpg_submit / kmcpg_search_batch / kmcpg_group_device; the call waits for the device to go idle): segments of 2 .. 512
 * matches ordered by the wave class of the sort kernels, of up to 4096 by the workgroup class, longer ones left to the host, and the runs
 * of equal printed score that held matches of more than one member (the tie rule at work).  The host words count what the host half has
 * ordered itself since that launch (segments above 4096, every segment with KMCPG_DEVICE_FINALIZE=0 or through kmcpg_finalize).  Tests. */
typedef struct {
  uint64_t wave_segments, wg_segments, long_segments, device_mixed_runs;
  uint64_t host_segments, host_mixed_runs;
} kmcpg_set_order;
int kmcpg_last_set_order(kmcpg_db* db, kmcpg_set_order* out);
/* One host process, several GPUs (what a cgo host needs): the blocks are partitioned over `devices`, kmcpg_search_batch fans
 * every batch out to all of them from one host thread per GPU; the per-read hit lists of the shards are gathered on the first
 * GPU with RCCL (grouped ncclSend/ncclRecv over xGMI of exactly the bytes each shard produced; librccl is bound at run time)
 * and reach the host in one copy — the reference's concatenation of its per-block workers' replies (util-db-search.go:939-964).
 * When RCCL cannot serve (ordinals repeat — RCCL wants one rank per device —, no librccl, KMCPG_RCCL=0, its self-test at open
 * fails) the shards' lists are copied to the host one by one and merged there; kmcpg_exchange_info says which it is.
 * kmcpg_query_device is not available on such a handle. */
int kmcpg_open_devices(const char* db_dir, const int32_t* devices, int32_t n_devices, kmcpg_db** out);
/* "RCCL gather over N device(s)" / "host merge of the shards' hit lists (<reason>)" / "single device: no exchange step";
 * the string lives until the calling thread's next call of this function */
const char* kmcpg_exchange_info(const kmcpg_db* db);
/* A database LARGER than the HBM at hand, on one GPU (the reference searches any size through mmap / --low-mem,
 * util-db-search.go:1238-1280, :6975-7335; search.go:80): the index is cut into `passes` shards (the byte-balanced partition of
 * kmcpg_open with shard_count = passes; 0 = as few as fit the free HBM of `device`), and kmcpg_search_batch / kmcpg_submit
 * search every batch against one resident shard after the other — upload shard, K1 + K2, keep the hit tuples, next shard —
 * then finalize the concatenated hit lists once: results are those of a resident database.  The search of a batch runs inside
 * kmcpg_submit on such a handle (it blocks); the shard searched last stays resident for the next batch, so a batch costs
 * passes - 1 uploads (11-44 GB/s from the page cache): use large batches.  If the index fits (1 pass) this is kmcpg_open.
 * kmcpg_open itself reports an index that does not fit with KMCPG_ENOMEM and the bytes needed / free in the message. */
int kmcpg_open_paged(const char* db_dir, int32_t device, int32_t passes, kmcpg_db** out);
/* passes of a paged handle (0 for every other handle) and how many shard uploads it has done so far */
int kmcpg_paged_info(const kmcpg_db* db, int32_t* passes, uint64_t* uploads);
/* How many bases (read 1 + read 2) one batch may hold on this handle so that its device workspace fits beside the resident index
 * (K1 and the sort + unique of long queries take up to 24 B per base, query.cpp): a paged handle answers from the HBM it kept
 * free beside its largest shard, every other handle from what is free now; 0 = unknown.  A batch that does not fit is not an
 * error of kmcpg_search_batch either: it is searched as two halves (recursively) and answered as one result. */
int kmcpg_batch_hint(const kmcpg_db* db, uint64_t* max_bases);
int kmcpg_close(kmcpg_db* db);
const char* kmcpg_last_error(void);
int kmcpg_db_info(const kmcpg_db* db, kmcpg_info* info);
/* The k-mer sizes of the database, largest first (`ks` of __db.yml, util-db-info.go:50; one entry for most databases):
 * *n = how many there are, the first min(*n, cap) are written to ks.  kmcpg_search_batch walks them by itself
 * (util-db-search.go:764, :1016-1022); a host that drives kmcpg_query_device + kmcpg_finalize per shard repeats the
 * search of its unmatched queries with kmcpg_params.k set to the next entry. */
int kmcpg_db_ks(const kmcpg_db* db, int32_t* ks, int32_t cap, int32_t* n);
/* Header.Names/GSizes/Indices/Sizes of one column (serialization.go:73-79) */
int kmcpg_col_info(const kmcpg_db* db, uint32_t col, const char** name, uint32_t* target_idx, uint64_t* gsize,
                   uint64_t* size);

/* -- the whole per-query pipeline for a batch of queries: replaces UnikIndexDB.handleQuery
 *    (util-db-search.go:763-1025) and the sorting/top-N of handleQuerySingleDB (:260-345).
 *    seqs/offs: read i is seqs[offs[i]..offs[i+1]) (ASCII, as fastx delivers it);
 *    seqs2/offs2: mates for paired-end input or NULL. */
int kmcpg_search_batch(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const uint8_t* seqs2,
                       const uint64_t* offs2, uint32_t n_reads, const kmcpg_params* params, kmcpg_result* out);
void kmcpg_result_free(kmcpg_result* r);

/* -- the same pipeline, asynchronous: the reference keeps 30 x threads queries in flight (util-db-search.go:243, :347-351);
 *    here a few BATCHES are.  kmcpg_submit copies the batch into pinned staging (the caller's buffers are free again when it
 *    returns), enqueues H2D copy, kernels and D2H copy on the handle's private stream and returns.  It never blocks: with all
 *    lanes (KMCPG_INFLIGHT, default 4) in flight it fails with KMCPG_EBUSY and the caller waits for one of its tickets first
 *    (kmcpg_search_batch waits for a lane instead, so a thread must not call it while it holds every lane itself).
 *    kmcpg_wait blocks until that batch's GPU work is done and runs the host half (float64 thresholds, FPR, sorting;
 *    --try-se / smaller-k retries) on the calling thread while later batches occupy the GPU.
 *    Tickets may be waited for in any order and from any thread; kmcpg_wait consumes the ticket, also when it fails.
 *    kmcpg_close refuses (KMCPG_EBUSY) while tickets are outstanding.
 *    kmcpg_search_batch(...) == kmcpg_submit(...) + kmcpg_wait(...). */
typedef struct kmcpg_ticket kmcpg_ticket;
int kmcpg_submit(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const uint8_t* seqs2, const uint64_t* offs2,
                 uint32_t n_reads, const kmcpg_params* params, kmcpg_ticket** out);
int kmcpg_wait(kmcpg_ticket* ticket, kmcpg_result* out);

/* -- the GPU half only (k-mer generation + COBS query on the local blocks), device-resident in and
 *    out: generateKmers (util-db-search.go:1037-1107) + dedup (:874-908) + the UnikIndex workers
 *    (:6611-7742, integer thresholds only).  All pointers are DEVICE pointers; `stream` is a
 *    hipStream_t (NULL = default stream).  d_counters points at TWO 64-bit words: [0] receives the number of hits
 *    produced (which may exceed hit_cap: then only hit_cap were stored and the caller retries with a larger buffer), [1] the
 *    largest NumKmers of the batch — if it exceeds what max_read_len allows (max_read_len - k + 1, twice that for pairs),
 *    max_read_len was under-reported, the match counters may have wrapped and the hits must be discarded.
 *    d_qkmers[i] receives NumKmers of read i (0 if not searched), d_qlen[i] its QueryLen.
 *    max_read_len must be >= the longest read (mate) of the batch: it sizes the counters.  The call only enqueues work on
 *    `stream` for short-read batches; when a query may exceed 32 768 k-mers — or 2048, in a batch too small to fill the GPU
 *    by itself — it reads 8 bytes back (which queries are long is known only on the device; they may take the chunked form of
 *    the kernel) and therefore synchronises the stream once or twice.
 *    The hit list depends on params->min_qcov, min_matched AND max_fpr (see kmcpg_hit: counts that cannot pass -f are left out
 *    on the device): finalize it with the SAME params — a looser max_fpr/min_qcov in kmcpg_finalize cannot bring back what
 *    the GPU already dropped (a stricter one is fine, kmcpg_finalize applies every threshold again). */
int kmcpg_query_device(kmcpg_db* db, const uint8_t* d_seqs, const uint64_t* d_offs, const uint8_t* d_seqs2,
                       const uint64_t* d_offs2, uint32_t n_reads, uint64_t total_bases, uint32_t max_read_len,
                       const kmcpg_params* params, kmcpg_hit* d_hits, uint64_t hit_cap, uint64_t* d_counters,
                       int32_t* d_qkmers, int32_t* d_qlen, void* stream);

/* -- the host half: thresholds that need float64/FPR (util-db-search.go:7471-7489), Match values,
 *    sorting, --keep-top-scores.  `hits` may be the concatenation of the hit lists of all shards
 *    (any order).  Every rank knows every column's metadata, so this can run on the gathering rank.
 *    `params` must not be looser (max_fpr, min_qcov, min_matched) than the ones the hits were produced with by
 *    kmcpg_query_device, which already filters on them. */
int kmcpg_finalize(const kmcpg_db* db, const kmcpg_hit* hits, uint64_t n_hits, const int32_t* qkmers,
                   const int32_t* qlen, uint32_t n_reads, const kmcpg_params* params, kmcpg_result* out);

/* -- the host half split in two (round 4): its grouping, -T filter and per-query ordering run on the GPU, the host only expands
 *    (column, count) pairs to Match records.  kmcpg_search_batch / kmcpg_submit use this by themselves (KMCPG_DEVICE_FINALIZE=0
 *    keeps the hits on the round-3 path through kmcpg_finalize); a host that drives kmcpg_query_device per shard gathers the
 *    shards' hit lists on one GPU (RCCL) and calls kmcpg_group_device there.
 *    kmcpg_group_device: d_hits[0 .. min(*d_n_hits, hit_cap)) as kmcpg_query_device left them (any order, any number of shards
 *    concatenated) -> d_pairs: the matches of read i at [d_read_offs[i], d_read_offs[i+1]), those failing -T (count / size <
 *    min_tcov in float64, util-db-search.go:7471-7473) dropped, ordered as handleQuerySingleDB orders them (:260-283, :105-145:
 *    -s qcov/tcov/jacc, ties by column; -S: column order).  Segments longer than 4096 matches come back grouped but unordered
 *    (kmcpg_finalize_grouped sorts those).  d_pairs needs room for hit_cap pairs, d_read_offs for n_reads + 2 words: the last
 *    one receives the number of hits that named a read or column that does not exist (must be 0).  Only enqueues on `stream`.
 *    kmcpg_finalize_grouped: the float64 Match values (qCov, tCov, jacc :7487-7489), the FPR column and its -f test (:7474-7478),
 *    --keep-top-scores (:285-311) and the name-independent metadata; same result as kmcpg_finalize on the same hits.  Segments
 *    that are not in that order (longer than 4096 matches, or a list that did not come from kmcpg_group_device) are sorted here. */
typedef struct {
  uint32_t col;   /* global column */
  uint32_t count; /* matched k-mers */
} kmcpg_pair;
/* -- compact results (round 5): on a database full of close relatives a read has hundreds of matches, and writing a 56-byte Match
 *    record for each (1.5 GB per 131 072 reads) was what bounded kmcpg_search_batch (6.8 M reads/s against 12.7 M for the kernels).
 *    The *_pairs forms return the FINAL matches of every query — every threshold, -f and --keep-top-scores applied, in the order
 *    kmcp search prints them — as 8-byte (column, mKmers) pairs; match_offs[i+1] - match_offs[i] is the query's `hits` column.
 *    Reference counterpart: the Match structs a worker appends (util-db-search.go:7479-7489) and the row loop that prints them
 *    (search.go:517-575) — here the second is what needs the first, one query at a time.
 *    kmcpg_expand_pairs derives the Match records of one query's pairs (qCov, tCov, jacc util-db-search.go:7487-7489, the FPR column
 *    util-fpr.go:32-50, column metadata) on the caller's thread, typically into a small scratch array right before the rows are formatted: the same bits as
 *    kmcpg_search_batch / kmcpg_wait would have written.  Everything else (arguments, errors, ownership: kmcpg_result_pairs_free)
 *    is as for the record forms; a ticket is consumed by EITHER kmcpg_wait or kmcpg_wait_pairs. */
typedef struct {
  uint32_t n_reads;
  int32_t k;
  int32_t* qlen;
  int32_t* qkmers;
  int32_t* ksize;
  uint64_t* match_offs;  /* [n_reads+1] */
  kmcpg_pair* pairs;     /* [match_offs[n_reads]] */
  void* owner;           /* internal */
} kmcpg_result_pairs;
/* -- packed queries (round 6): long queries (genomes, contigs, HiFi reads) as 2-bit codes.  A batch of 256 assemblies is 1 GB of ASCII;
 *    kmcpg_submit reads it once more to pack it into pinned staging (at 29 k genomes/s the host reads 117 GB/s of text for that).  A reader
 *    that packs where it first touches the bases (kmcp-search -g does: cli/kmcp_search.cpp) hands the library a quarter of the bytes and no
 *    second pass.  Reference counterpart of the input: the sequence a Query carries (util-db-search.go:50-57, search.go:885-915 for -g).
 *    Layout: base j of the batch (all queries back to back, offs in BASES as for kmcpg_submit) sits in bits 2*(j % 4) of codes[j / 4];
 *    code = (ascii >> 1) & 3, i.e. A/a 0, C/c 1, T/t/U/u 2, G/g 3.  Every other byte (N, IUPAC codes, gaps ...) is listed as a run
 *    {first base, length, the byte}: it reaches the k-mer kernels verbatim (its code bits are ignored).  Runs must lie inside the batch and
 *    must not overlap.  Exactness: the k-mer kernels see a base only through the ntHash seed tables, where all spellings of a base share an
 *    entry (kmcp_amd/csrc/pack2.hpp) — results are those of kmcpg_submit on the text, bit for bit (tests/test_gpu_pack.py).
 *    Single-end only.  Handles that must re-read the text (several k-mer sizes, paged indexes) unpack it on the host first: correct, slower.
 *    kmcpg_pack2 appends n bases of text at base position `pos` of a codes array (any alignment; codes needs (pos + n + 3) / 4 + 8 bytes)
 *    and writes the runs it met to exc[*n_exc ...] (positions absolute); when exc_cap is too small it returns KMCPG_ENOMEM with *n_exc =
 *    the number needed in total (call again with room: packing the same bases twice is harmless).  kmcpg_unpack2 is its inverse
 *    (canonical spelling A C G T for the coded bases). */
typedef struct {
  uint64_t pos;  /* first base of the run (position in the batch) */
  uint32_t len;
  uint32_t byte; /* the ASCII byte of every base of the run */
} kmcpg_exc_run;
int kmcpg_pack2(const uint8_t* seq, uint64_t n, uint64_t pos, uint8_t* codes, kmcpg_exc_run* exc, uint64_t exc_cap, uint64_t* n_exc);
/* Page-locked host memory for a reader's batches.  Codes that live in memory from kmcpg_host_alloc are uploaded from where they are —
 * kmcpg_submit_packed makes no staging copy of them (a quarter of a gigabyte per batch of 256 assemblies: the copy took longer than the GPU
 * needs for the batch) — and must then stay untouched until kmcpg_wait / kmcpg_wait_pairs has returned for the ticket.  Codes in any other
 * memory are copied inside the call as every other input is.  (offs and exc are small and always copied.) */
int kmcpg_host_alloc(uint64_t bytes, void** out);
int kmcpg_host_free(void* p);
int kmcpg_unpack2(const uint8_t* codes, uint64_t n_bases, const kmcpg_exc_run* exc, uint64_t n_exc, uint8_t* out);
int kmcpg_submit_packed(kmcpg_db* db, const uint8_t* codes, const uint64_t* offs, const kmcpg_exc_run* exc, uint64_t n_exc, uint32_t n_reads,
                        const kmcpg_params* params, kmcpg_ticket** out);

/* -- sliding windows of long reads and contigs: what `seqkit sliding -s step -W window [-g] | kmcp search` computes (the reference's
 *    advice for long queries, search.go:59-61), without the window text.  Every read (single-end) yields windows i = 0, step, 2 step, ...
 *    ending at e = i + window; with greedy a window that runs over the end is cut there (e = L) and windows go on while i < L, without it
 *    they stop at the first such window (a read shorter than `window` has none).  Each window is an ordinary query (qlen e - i, -m, -u,
 *    multi-k retries, -K, -n, -s / -S, -f apply per window); the result has ONE ROW PER WINDOW, read by read, start ascending, and is
 *    consumed by kmcpg_wait / kmcpg_wait_pairs as any other ticket.  The bases of each read are uploaded once and the k-mer kernels read a
 *    window's bases in place (windows.hip, k1_device.hpp) on single-device handles; paged (kmcpg_open_paged) and multi-device
 *    (kmcpg_open_devices) handles, and databases with several k-mer sizes searched without an explicit k, cut the windows into text on
 *    the host and search that (same results).  Windows that do not fit one batch of the handle (kmcpg_batch_hint, in window bases) are
 *    cut into pieces by the library — a read's windows may span several — and the ticket answers for all of them. */
typedef struct {
  uint64_t step;   /* -s, >= 1 */
  uint64_t window; /* -W, >= 1 */
  int32_t greedy;  /* -g */
  int32_t reserved;
} kmcpg_window_spec;
int kmcpg_submit_windows(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, uint32_t n_reads, const kmcpg_window_spec* spec,
                         const kmcpg_params* params, kmcpg_ticket** out);
int kmcpg_submit_packed_windows(kmcpg_db* db, const uint8_t* codes, const uint64_t* offs, const kmcpg_exc_run* exc, uint64_t n_exc,
                                uint32_t n_reads, const kmcpg_window_spec* spec, const kmcpg_params* params, kmcpg_ticket** out);
/* how many windows the reads of offs[0 .. n_reads] yield and how many bases they hold together (the `bases` kmcpg_batch_hint speaks of) */
int kmcpg_window_count(const uint64_t* offs, uint32_t n_reads, const kmcpg_window_spec* spec, uint64_t* n_windows, uint64_t* window_bases);
/* result rows first .. first + n - 1 of such a batch -> the read (index into offs) and the 0-based first base of each window */
int kmcpg_window_locate(const uint64_t* offs, uint32_t n_reads, const kmcpg_window_spec* spec, uint64_t first, uint64_t n, uint32_t* read,
                        uint64_t* start);

int kmcpg_search_batch_pairs(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const uint8_t* seqs2, const uint64_t* offs2,
                             uint32_t n_reads, const kmcpg_params* params, kmcpg_result_pairs* out);
int kmcpg_wait_pairs(kmcpg_ticket* ticket, kmcpg_result_pairs* out);
void kmcpg_result_pairs_free(kmcpg_result_pairs* r);
int kmcpg_expand_pairs(const kmcpg_db* db, int32_t qkmers, const kmcpg_pair* pairs, uint64_t n, kmcpg_match* out);

int kmcpg_group_device(kmcpg_db* db, const kmcpg_hit* d_hits, const uint64_t* d_n_hits, uint64_t hit_cap, const int32_t* d_qkmers,
                       uint32_t n_reads, const kmcpg_params* params, kmcpg_pair* d_pairs, uint64_t* d_read_offs, void* stream);
int kmcpg_finalize_grouped(const kmcpg_db* db, const kmcpg_pair* pairs, const uint64_t* read_offs, const int32_t* qkmers,
                           const int32_t* qlen, uint32_t n_reads, const kmcpg_params* params, kmcpg_result* out);

/* -- species-specific queries (K4, k4_specific.hip): the decision of `kmcp utils filter` (kmcp/cmd/filter.go:306-391) on K3's output,
 *    which is in device memory grouped by read.  A query is specific when its matches name ONE target, or — with a species table — when
 *    all its targets lie under one species (kmcp_amd/csrc/specific_rule.hpp states the rule and why it equals the reference's "LCA at
 *    or below rank species").  Each global column carries two integers: target_class, equal exactly for the columns of one printed
 *    target, and species_class, the species TaxId the target lies under, or 0.
 *    The state lives on the handle, not in kmcpg_params.  kmcpg_set_specific uploads the tables (n_cols must be the handle's column count,
 *    over all members for a kmcpg_open_set handle); species_class == NULL is strain / assembly level (one target only);
 *    (NULL, NULL, 0) switches the stage off and frees the tables.  KMCPG_EUNSUPPORTED: paged, multi-device and sharded handles.
 *    kmcpg_specific_device runs the stage alone, as kmcpg_group_device runs K3: d_pairs / d_read_offs as kmcpg_group_device wrote them
 *    (d_read_offs[n_reads] pairs, at most pair_cap), d_qkmers as kmcpg_query_device wrote them.  Read i gets d_verdicts[i]:
 *    KMCPG_SPECIFIC_KEEP (its pairs are copied to d_out_pairs[d_out_offs[i] .. d_out_offs[i + 1]) in their order; also every read without
 *    pairs), KMCPG_SPECIFIC_DROP (an empty segment) or KMCPG_SPECIFIC_HOST: reads of more than final_n k-mers keep all their pairs and are
 *    judged by the host after its own -f test (their matches may still fall there; for the library's own batches final_n is the
 *    largest query whose matches are final on the device).  d_out_pairs needs room for out_cap >= the input's pairs, d_out_offs for
 *    n_reads + 1 words, d_verdicts for n_reads bytes; the outputs must not overlap the inputs.  Only enqueues on `stream`.
 *    kmcpg_last_specific: the witness of the handle's last K4 launch (the call waits for the device to go idle): reads WITH pairs that
 *    were kept, dropped, left to the host; pairs in and out; segments judged by a lane group (up to 64 pairs) and by a whole wave;
 *    segments that did not lie inside pair_cap (treated as empty; must be 0); and, at profiling level >= 1, the HIP-event time of the
 *    stage's kernels and one record per kernel launched, in launch order (*n_launches = 0 otherwise, and when no K4 launch has been made since the stage was set). */
#define KMCPG_SPECIFIC_DROP 0
#define KMCPG_SPECIFIC_KEEP 1
#define KMCPG_SPECIFIC_HOST 2
int kmcpg_set_specific(kmcpg_db* db, const uint32_t* target_class, const uint32_t* species_class, uint32_t n_cols);
int kmcpg_specific_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers,
                          uint32_t n_reads, int32_t final_n, kmcpg_pair* d_out_pairs, uint64_t out_cap, uint64_t* d_out_offs,
                          uint8_t* d_verdicts, void* stream);
enum { KMCPG_K4_VERDICT = 0, KMCPG_K4_SCAN_TILES, KMCPG_K4_SCAN_SUMS, KMCPG_K4_SCAN_ADD, KMCPG_K4_COMPACT, KMCPG_K4_KERNELS };
typedef struct {
  int32_t kernel;       /* KMCPG_K4_* */
  uint32_t grid, block; /* workgroups, threads per workgroup */
  int32_t cls;          /* segment classes the launch serves: bit 0 lane groups (up to 64 pairs), bit 1 whole waves; 0 for the scan */
} kmcpg_k4_launch;
typedef struct {
  uint64_t kept, dropped, host;               /* reads with pairs, by verdict */
  uint64_t pairs_in, pairs_out;
  uint64_t group_segments, wave_segments;     /* segments judged on the device, by size class */
  uint64_t bad_segments;
  double k4_ms;                               /* HIP-event time of the stage's kernels at profiling level >= 1; -1 otherwise */
} kmcpg_specific_stats;
int kmcpg_last_specific(kmcpg_db* db, kmcpg_specific_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches);

/* -- window summaries for region merging (K5, k5_summary.hip): what `kmcp utils merge-regions` derives from the rows of one query before
 *    it merges (kmcp/cmd/merge-regions.go:256-279; kmcp_amd/csrc/regions_rule.hpp states the rule): n_targets = the distinct targets among
 *    the window's surviving matches (0: no rows — unmatched, or dropped by K4), score = the printed qCov ("%.4f", parsed back) of the
 *    first row of each distinct target, added in print order in float64 and divided by n_targets when it is above 1.  Bit for bit what
 *    kmcp-regions computes from the TSV rows of the window.
 *    kmcpg_summarize_device runs the stage alone on device pointers, as kmcpg_specific_device runs K4, whose outputs it takes: d_pairs /
 *    d_offs = the surviving segments (at most pair_cap pairs), d_verdicts, d_qkmers, n windows; the tables are those of
 *    kmcpg_set_specific (KMCPG_EINVAL while the stage is off).  Window i gets d_out[i].  A window the device does not summarise — several
 *    targets among more than 64 pairs, and every window with verdict KMCPG_SPECIFIC_HOST, whose pairs still face the host's -f test — has
 *    flags = KMCPG_SUMMARY_LEFT (| KMCPG_SUMMARY_HOST), n_targets = the number of its pairs, and its pairs, and only those, are copied to d_left_pairs[d_left_offs[i] ..
 *    d_left_offs[i + 1]) in their order (d_left_offs: n + 1 words; left_cap >= pair_cap).  A window of one target is summarised on the
 *    device at any length.  Only enqueues on `stream`.
 *    kmcpg_last_summary: the witness of the handle's last K5 launch (the call waits for the device to go idle): windows summarised as a
 *    single target, by the wave (several targets), left to the host, and empty or dropped — the four add up to the windows —; the pairs
 *    of the LEFT windows; segments that did not lie inside pair_cap (treated as empty; must be 0); and, at profiling level >= 1, the
 *    HIP-event time of the stage's kernels and one record per kernel launched (the scan's records carry KMCPG_K4_SCAN_*). */
#define KMCPG_SUMMARY_LEFT 1u
#define KMCPG_SUMMARY_HOST 2u  /* with LEFT: the window's verdict was KMCPG_SPECIFIC_HOST */
typedef struct {
  uint32_t n_targets;  /* LEFT (kmcpg_summarize_device only): the number of the window's pairs in d_left_pairs */
  uint32_t flags;      /* bit 0: KMCPG_SUMMARY_LEFT, bit 1: KMCPG_SUMMARY_HOST; 0 in every record of kmcpg_wait_summaries */
  double score;
} kmcpg_window_summary;
enum { KMCPG_K5_SUMMARY = 16, KMCPG_K5_COMPACT = 17 };  /* kmcpg_k4_launch.kernel of K5's own kernels */
typedef struct {
  uint64_t single, wave, left, empty;  /* windows by the class they took */
  uint64_t left_pairs;                 /* pairs of the LEFT windows (kmcpg_wait_summaries: downloaded for them) */
  uint64_t bytes_d2h;                  /* kmcpg_wait_summaries: bytes that came from the device for the ticket; 0 after kmcpg_summarize_device */
  uint64_t bad_segments;
  double k5_ms;                        /* HIP-event time of the stage's kernels at profiling level >= 1; -1 otherwise */
} kmcpg_summary_stats;
int kmcpg_summarize_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_offs, uint64_t pair_cap, const uint8_t* d_verdicts,
                           const int32_t* d_qkmers, uint32_t n, kmcpg_window_summary* d_out, kmcpg_pair* d_left_pairs, uint64_t left_cap,
                           uint64_t* d_left_offs, void* stream);
int kmcpg_last_summary(kmcpg_db* db, kmcpg_summary_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches);
/*    kmcpg_submit_windows_summary: kmcpg_submit_windows with the species-specific stage ON (KMCPG_EINVAL while it is off) and K5 behind
 *    it: the result is one summary per window instead of its matches — what `kmcp-search --regions-bed` merges into regions.  Per window
 *    16 bytes of summary and its qlen / qkmers leave the GPU, no pairs and no offsets; the windows the device LEFT have their pairs
 *    downloaded and are summarised by the host half (its -f test, the rule of specific_rule.hpp where the verdict was HOST, then
 *    regions_rule.hpp), so every record the caller sees is final and has flags = 0.  KMCPG_EUNSUPPORTED as for the stage (try_se,
 *    top_n_scores != 0, several k-mer sizes with k == 0) and on database sets.  Windows cut into pieces, KMCPG_WINDOWS_HOST=1 (window
 *    text), KMCPG_SPECIFIC_DEVICE=0 (every window with matches LEFT) and KMCPG_DEVICE_FINALIZE=0 (no K3: the summaries come from the
 *    finished records) give the same records.  The ticket is consumed by kmcpg_wait_summaries ONLY: kmcpg_wait and kmcpg_wait_pairs
 *    refuse it (KMCPG_EINVAL, the ticket stays valid), and kmcpg_wait_summaries refuses every other ticket.  kmcpg_submit_windows and
 *    kmcpg_submit_packed_windows keep refusing a handle with the stage on.  After kmcpg_wait_summaries kmcpg_last_summary reports the
 *    TICKET: its windows by who summarised them (single / wave: the device, left: the host, empty: no rows), the pairs downloaded for
 *    the LEFT windows and the bytes that came from the device. */
typedef struct {
  uint32_t n_windows;
  uint32_t reserved;
  int32_t* qlen;
  int32_t* qkmers;
  kmcpg_window_summary* s;  /* [n_windows] */
  void* owner;              /* internal */
} kmcpg_result_summaries;
int kmcpg_submit_windows_summary(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, uint32_t n_reads, const kmcpg_window_spec* spec,
                                 const kmcpg_params* params, kmcpg_ticket** out);
int kmcpg_wait_summaries(kmcpg_ticket* ticket, kmcpg_result_summaries* out);
void kmcpg_result_summaries_free(kmcpg_result_summaries* r);

/* -- reference statistics (K6, k6_refstats.hip): what stage 1/4 of `kmcp profile` counts per reference (kmcp/cmd/profile.go:761-1099;
 *    kmcp_amd/csrc/refstats_rule.hpp states the rule), on K3's output while it is in device memory.  Every global column — a chunk of a
 *    reference — has four counters: rows (matches of the column), firsts (queries whose first row of the column's target is this column),
 *    ureads (of those, the queries that name one target or — with a species table — one species), hic_ureads (of those, the ones whose
 *    printed qCov of that first row is >= hic_min_qcov).  The tables are those of kmcpg_set_specific but the stage's own: it does NOT
 *    filter, the result of every call is byte for byte what it is with the stage off, and both stages may be on together.
 *    kmcpg_set_refstats uploads the tables and allocates zeroed counters; (NULL, NULL, 0, 0) switches the stage off and frees them.
 *    KMCPG_EUNSUPPORTED as for kmcpg_set_specific: paged, multi-device and sharded handles; while the stage is on, batches with try_se,
 *    top_n_scores != 0 or several k-mer sizes with k == 0, and every window submit.
 *    While the stage is on, every batch of kmcpg_submit / kmcpg_search_batch (and their _pairs / _packed forms) is counted: on the device
 *    behind K3 — as the batch's last kernel, after K4 where that stage is on too: K6 reads K3's pairs, which K4 leaves where they are —
 *    for the reads whose matches are final there, by the host half at wait time for the others (queries of more k-mers
 *    than the device's -f bound covers, segments above 4096 pairs, several targets among more than 64 pairs; KMCPG_DEVICE_FINALIZE=0:
 *    every read) — its own -f test first, then the same rule.  A batch that is run again because its hit buffer overflowed is counted once
 *    (totals.skipped_launches counts the launches that left the counting to the rerun).  A kmcpg_search_batch call whose pieces fail part
 *    of the way and which is then searched again as a whole marks the counters as a failed batch does (below).
 *    kmcpg_refstats_read waits for the device and adds device and host counters; valid once every ticket has been waited for.
 *    KMCPG_EDEVICE if a batch failed after its reads had been counted (call kmcpg_refstats_reset).  totals may be NULL.
 *    kmcpg_refstats_device runs K6 alone on device pointers, as kmcpg_specific_device runs K4: d_left[i] = 1 for the reads it does not
 *    count (n_reads bytes).  d_n_hits may be NULL; otherwise the launch counts nothing when *d_n_hits > hit_cap (the batch will be run
 *    again).  Only enqueues on `stream`.
 *    kmcpg_last_refstats: the witness of the handle's last K6 launch (the call waits for the device to go idle; one set of witness words
 *    per handle, zeroed by every launch: meaningful only with ONE batch in flight — the counters themselves are not affected): reads by class, adds to
 *    the workgroups' LDS tables, adds to global memory (table flushes and spills) and the spills among them, whether the overflow guard
 *    skipped the launch, segments outside pair_cap (must be 0), the grid and the table size; at profiling level >= 1 the HIP-event
 *    time and one launch record.  KMCPG_REFSTATS_SLOTS (read by kmcpg_set_refstats): slots of a workgroup's table, a power of two up to
 *    2048, 0 = no table. */
typedef struct {
  uint64_t rows, firsts, ureads, hic_ureads;
} kmcpg_col_stats;
typedef struct {
  uint64_t matched_reads, unique_reads;  /* queries with at least one row; of those the unique ones */
  uint64_t host_reads;                   /* of matched_reads, counted by the host half */
  uint64_t skipped_launches;             /* K6 launches that counted nothing because the batch's hit buffer had overflowed (the rerun counted) */
} kmcpg_refstats_totals;
enum { KMCPG_K6_REFSTATS = 32 };  /* kmcpg_k4_launch.kernel of K6's kernel */
typedef struct {
  uint64_t empty, single, wave, left;            /* reads by the class they took; the four add up to the reads */
  uint64_t lds_adds, global_adds, spilled_adds;  /* spilled_adds is part of global_adds */
  uint64_t skipped;                              /* 1: the overflow guard skipped the launch */
  uint64_t bad_segments;
  uint32_t grid, slots;
  double k6_ms;                                  /* HIP-event time of the kernel at profiling level >= 1; -1 otherwise */
} kmcpg_refstats_stats;
int kmcpg_set_refstats(kmcpg_db* db, const uint32_t* target_class, const uint32_t* species_class, uint32_t n_cols, double hic_min_qcov);
int kmcpg_refstats_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers,
                          uint32_t n_reads, int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left, void* stream);
int kmcpg_refstats_read(kmcpg_db* db, kmcpg_col_stats* out, uint32_t n_cols, kmcpg_refstats_totals* totals);
int kmcpg_refstats_reset(kmcpg_db* db);
int kmcpg_last_refstats(kmcpg_db* db, kmcpg_refstats_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches);

/* -- shared reads of reference pairs (K7, k7_cooccur.hip): what stage 2/4 of `kmcp profile` counts (kmcp/cmd/profile.go:1117-1279;
 *    kmcp_amd/csrc/cooccur_rule.hpp states the rule), on K3's output while it is in device memory.  A pair is an unordered pair of printed
 *    targets (target_class: chunks of one genome are one target, as for kmcpg_set_refstats); its count is the number of queries whose
 *    final matches name both.  The stage does NOT filter: the result of every call is byte for byte what it is with the stage off.
 *    kmcpg_set_cooccur uploads its own copy of the class table and allocates the zeroed pair table (open-addressed in device memory, 16
 *    bytes per slot; table_slots must be a power of two up to 2^30, 0 = the default of 2^21 slots, 32 MiB); it is independent of
 *    kmcpg_set_refstats and kmcpg_set_specific, and (NULL, 0, 0) switches it off and frees everything.  KMCPG_EUNSUPPORTED as for
 *    kmcpg_set_refstats: paged, multi-device and sharded handles; while the stage is on, batches with try_se, top_n_scores != 0 or several
 *    k-mer sizes with k == 0, and every window submit.
 *    While the stage is on, every batch of kmcpg_submit / kmcpg_search_batch (and their _pairs / _packed forms) is counted: on the device
 *    behind K3 — as the batch's last kernel, after K4 and K6 where those are on — for the reads whose matches are final there, by the
 *    host half at wait time, into a host map, for the others (queries of more k-mers than the device's -f bound covers, segments above
 *    4096 pairs, several targets among more than 64 pairs, reads whose pairs found no room in the table; KMCPG_COOCCUR_DEVICE=0 or
 *    KMCPG_DEVICE_FINALIZE=0: every read) — its own -f test first, then the same rule.  A read is counted completely or not at all: a
 *    full table never loses or half-counts one (it goes to the host half).  The table does not grow; size it with table_slots.  A batch
 *    that is run again because its hit buffer overflowed is counted once.
 *    kmcpg_cooccur_read waits for the device and merges the device slots with a count > 0 and the host map: n_pairs records sorted by
 *    (class_a, class_b), class_a < class_b, the first `cap` of them in out_pairs (cap too small: *n_pairs says how many there are, and
 *    the call can be repeated).  Valid once every ticket has been waited for.  KMCPG_EDEVICE if a batch failed after its reads had been
 *    counted, or a kmcpg_search_batch call's pieces failed part of the way (call kmcpg_cooccur_reset).  totals may be NULL.
 *    kmcpg_cooccur_device runs K7 alone on device pointers, as kmcpg_refstats_device runs K6: d_left[i] = 1 for the reads it does not
 *    count (n_reads bytes).  d_n_hits may be NULL; otherwise the launch counts nothing when *d_n_hits > hit_cap.  max_wgs: 0 = the
 *    handle's (two workgroups per CU), fewer to force grid-stride rounds.  Only enqueues on `stream`.
 *    kmcpg_last_cooccur: the witness of the handle's last K7 launch (the call waits for the device to go idle; one set of witness words
 *    per handle, zeroed by every launch: meaningful only with ONE batch in flight).  KMCPG_COOCCUR_SLOTS (read by kmcpg_set_cooccur):
 *    slots of a workgroup's LDS table, a power of two up to 4096 (anything else is KMCPG_EINVAL), 0 = no LDS table; default 2048. */
typedef struct {
  uint32_t class_a, class_b;  /* class_a < class_b */
  uint64_t reads;
} kmcpg_cooccur_pair;
typedef struct {
  uint64_t multi_reads;              /* queries with several targets, counted by either half */
  uint64_t device_adds, host_adds;   /* pair adds (one per read and pair) by the device and by the host half */
  uint64_t left_full;                /* reads the device left to the host because their pairs found no room in the table */
  uint64_t host_reads;               /* of multi_reads, counted by the host half */
  uint64_t skipped_launches;         /* K7 launches that counted nothing because the batch's hit buffer had overflowed (the rerun counted) */
  uint64_t table_slots, keys;        /* the table's size, and its keys (with any count) */
  uint64_t rebuilds;                 /* always 0: the table does not grow */
} kmcpg_cooccur_totals;
enum { KMCPG_K7_COOCCUR = 48 };  /* kmcpg_k4_launch.kernel of K7's kernel */
typedef struct {
  uint64_t empty, single, wave, left;            /* reads by the class they took; the four add up to the reads */
  uint64_t left_full;                            /* of left: no room in the table */
  uint64_t pairs;                                /* pairs enumerated (of the reads counted) = lds_adds + the adds straight to global memory */
  uint64_t lds_adds, global_adds, spilled_adds;  /* global_adds: table flushes and adds past the LDS table; spilled_adds: of those, past a FULL LDS table */
  uint64_t claimed;                              /* keys claimed in the table in device memory */
  uint64_t skipped;                              /* 1: the overflow guard skipped the launch */
  uint64_t bad_segments;
  uint32_t grid, slots;
  double k7_ms;                                  /* HIP-event time of the kernel at profiling level >= 1; -1 otherwise */
} kmcpg_cooccur_stats;
int kmcpg_set_cooccur(kmcpg_db* db, const uint32_t* target_class, uint32_t n_cols, uint64_t table_slots);
int kmcpg_cooccur_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers,
                         uint32_t n_reads, int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left, uint32_t max_wgs, void* stream);
int kmcpg_cooccur_read(kmcpg_db* db, kmcpg_cooccur_pair* out_pairs, uint64_t cap, uint64_t* n_pairs, kmcpg_cooccur_totals* totals);
int kmcpg_cooccur_reset(kmcpg_db* db);
int kmcpg_last_cooccur(kmcpg_db* db, kmcpg_cooccur_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches);

/* -- recount with ambiguity correction (K8, k8_recount.hip): stage 3/4 of `kmcp profile` (kmcp/cmd/profile.go:1282-1888;
 *    kmcp_amd/csrc/recount_rule.hpp states the rule: the order of a read's targets, the elimination loop in bit masks, the integer shares).
 *    Every global column has four counters IN UNITS: match, uniq, hic (units of 1 / 720720 read) and bases (units of 2^-16 base).  Stage 3
 *    needs the final verdicts of stage 1 and the final pair list of stage 2, so it runs in two steps: while the stage is on, every batch is
 *    LOGGED behind K3 (k8_log: reads with one target are counted at once, reads with several targets among up to 64 pairs are appended to
 *    a read log in device memory, the others — more k-mers than the device's -f bound covers, more than 4096 pairs, several targets among
 *    more than 64 pairs, no room in the log — are appended by the host half at wait time, after its own -f test, to a log in host memory);
 *    after the last ticket was waited for, kmcpg_recount_run REPLAYS both logs (k8_replay on the device, the same rule on the host).
 *    The stage does NOT filter: the result of every call is byte for byte what it is with the stage off.
 *    kmcpg_set_recount uploads its own copies of the class tables (species_class NULL: strain / assembly level) and allocates the zeroed
 *    counters and the read log: log_bytes of device memory, fixed until the stage is set again (64 bytes .. 4 GiB; 0 = the default of
 *    256 MiB; a read with m pairs takes 8 * (m + 3) bytes).  A read is logged completely or not at all; the log does not grow.  It is
 *    independent of kmcpg_set_refstats, kmcpg_set_cooccur and kmcpg_set_specific; (NULL, NULL, 0, 0, 0) switches it off and frees
 *    everything.  KMCPG_EUNSUPPORTED as for kmcpg_set_refstats: paged, multi-device and sharded handles; while the stage is on, batches with
 *    try_se, top_n_scores != 0 or several k-mer sizes with k == 0, and every window submit.  A batch that is run again because its hit
 *    buffer overflowed is logged once.
 *    kmcpg_recount_log_device runs k8_log alone on device pointers, as kmcpg_cooccur_device runs K7, with d_qlen (one int32 per read)
 *    beside d_qkmers: d_left[i] = 1 for the reads it neither counts nor logs.  Only enqueues on `stream`.
 *    kmcpg_recount_run: classes[c] = {kept: stage 1's verdict of target class c is ok; reads, ureads: its stage-1 sums}, for every class
 *    of target_class; pairs = what kmcpg_cooccur_read returns (sorted by (class_a, class_b), class_a < class_b; anything else is
 *    KMCPG_EINVAL) — a pair that is not listed shares 0 reads.  params: one_minus_d = 1 - --min-dreads-prop, r_err = --max-mismatch-err,
 *    no_amb_corr, level_species.  It waits for the device, zeroes the replay counters and replays: the logs are kept, so the call can be
 *    repeated with other classes, pairs or params without a new search.  KMCPG_EDEVICE if a batch failed after it had been logged (call
 *    kmcpg_recount_reset and search again).
 *    kmcpg_recount_read: single-target reads of kept classes + device replay + host replay, n_cols records; valid after kmcpg_recount_run.
 *    kmcpg_last_recount: the witness of the handle's last k8_log launch and of the last replay (the call waits for the device to go idle;
 *    the words of k8_log are zeroed by every launch: meaningful only with ONE batch in flight).  KMCPG_RECOUNT_SLOTS (read by
 *    kmcpg_set_recount): slots of a workgroup's LDS table, a power of two up to 1024 (anything else is KMCPG_EINVAL), 0 = no table;
 *    default 1024.  KMCPG_RECOUNT_LOG_BYTES (read by kmcpg_set_recount): the log's size, whatever log_bytes says (the same range).
 *    KMCPG_RECOUNT_DEVICE=0 sends every read to the host half. */
typedef struct {
  uint64_t match, uniq, hic, bases;  /* units: 720720 per read, 65536 per base */
} kmcpg_recount_col;
typedef struct {
  uint32_t kept, reserved;
  uint64_t reads, ureads;
} kmcpg_recount_class;
typedef struct {
  double one_minus_d, r_err;
  uint32_t no_amb_corr, level_species;
} kmcpg_recount_params;
typedef struct {
  uint64_t recounted_reads, unique_reads, corrected_reads;  /* reads with a kept target; that ended with one target; that lost a target */
  uint64_t single_reads;                                    /* of recounted_reads, counted by k8_log at once */
  uint64_t replayed_reads, host_reads;                      /* reads replayed from the logs (with or without a kept target); of those, from the host log */
  uint64_t left_full;                                       /* reads the device left to the host for want of log room */
  uint64_t skipped_launches;                                /* k8_log launches that did nothing because the batch's hit buffer had overflowed */
  uint64_t log_bytes, log_bytes_used, logged_reads;         /* the device log */
} kmcpg_recount_totals;
enum { KMCPG_K8_LOG = 64, KMCPG_K8_REPLAY = 65 };  /* kmcpg_k4_launch.kernel of K8's kernels */
typedef struct {
  uint64_t empty, single, logged, left;          /* k8_log: reads by the class they took; the four add up to the reads */
  uint64_t left_full;                            /* of left: no room in the log */
  uint64_t lds_adds, global_adds, spilled_adds;  /* spilled_adds is part of global_adds */
  uint64_t skipped;                              /* 1: the overflow guard skipped the launch */
  uint64_t bad_segments;
  uint64_t log_bytes_used;                       /* the device log after the launch (the call waits) */
  uint64_t replay_reads, replay_recounted, replay_corrected, replay_unique;  /* k8_replay: reads; with a kept target; that lost one; that ended unique */
  uint64_t replay_lookups;                       /* binary searches in the pair list */
  uint64_t replay_lds_adds, replay_global_adds, replay_spilled_adds;
  uint32_t grid, slots, replay_grid, reserved;
  double log_ms, replay_ms;                      /* HIP-event times at profiling level >= 1; -1 otherwise */
} kmcpg_recount_stats;
int kmcpg_set_recount(kmcpg_db* db, const uint32_t* target_class, const uint32_t* species_class, uint32_t n_cols, double hic_min_qcov, uint64_t log_bytes);
int kmcpg_recount_log_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers,
                             const int32_t* d_qlen, uint32_t n_reads, int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_left,
                             uint32_t max_wgs, void* stream);
int kmcpg_recount_run(kmcpg_db* db, const kmcpg_recount_class* classes, uint32_t n_classes, const kmcpg_cooccur_pair* pairs, uint64_t n_pairs,
                      const kmcpg_recount_params* params);
int kmcpg_recount_read(kmcpg_db* db, kmcpg_recount_col* out_cols, uint32_t n_cols, kmcpg_recount_totals* totals);
int kmcpg_recount_reset(kmcpg_db* db);
int kmcpg_last_recount(kmcpg_db* db, kmcpg_recount_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches);

/* -- abundance estimation by EM (K9, k9_em.hip): one PASS of stage 4/4 of `kmcp profile` (kmcp/cmd/profile.go:1907-2570;
 *    kmcp_amd/csrc/em_rule.hpp states the rule: the integer shares of a read over its estimated targets, the two-word bases, the roll-up
 *    and the loop).  A pass works on what the recount stage keeps: the read log in device memory, the host log and the single-target
 *    counters; nothing is searched again.  Units: 2 952 069 120 (= 720720 << 12) per read; bases_lo / bases_hi hold the low 32 bits and the
 *    rest of exact products qlen * share, in units of 1 / 2 952 069 120 base: bases = (bases_hi * 2^32 + bases_lo) / 2 952 069 120.
 *    kmcpg_em_pass: classes[c] = {est: class c is in this pass's whitelist; coverage: its current coverage}, for every class of the
 *    recount stage's target_class.  KMCPG_EINVAL with the recount stage off, and for an estimated class whose coverage is not finite and
 *    > 0; KMCPG_EDEVICE after a tainted batch, as kmcpg_recount_run.  It waits for the device, zeroes its own pass counters (allocated on
 *    first use, freed with the recount stage), runs k9_em over the device log and the same rule over the host log.  It does not touch
 *    what kmcpg_recount_run / kmcpg_recount_read work on, and can be repeated with other classes without a new search.
 *    kmcpg_em_read: per column, the single-target reads' counters if the column's class is estimated (match, uniq, hic << 12; their bases
 *    apart, in units of 2^-16 base) plus both halves of the pass; valid after kmcpg_em_pass.
 *    kmcpg_last_em: the witness of the last k9_em launch (the call waits for the device to go idle).
 *    KMCPG_EM_SLOTS (read by kmcpg_em_pass): slots of a workgroup's LDS table, a power of two up to 1024 (anything else is KMCPG_EINVAL),
 *    0 = no table, every add is a global atomic; default 0.  The grid is bounded as K8's (KMCPG_RECOUNT_WGS). */
typedef struct {
  uint32_t est, reserved;
  double coverage;
} kmcpg_em_class;
typedef struct {
  uint64_t match, uniq, hic;    /* units of 1 / 2 952 069 120 read, single-target reads included */
  uint64_t single_bases;        /* the single-target reads' bases, units of 2^-16 base */
  uint64_t bases_lo, bases_hi;  /* the pass's bases, see above */
} kmcpg_em_col;
typedef struct {
  uint64_t assigned_reads;  /* reads with at least one estimated target */
  uint64_t unique_reads;    /* of those, with exactly one */
  uint64_t split_reads;     /* ... with several: shared out by coverage */
  uint64_t host_reads;      /* of assigned_reads, from the host log */
} kmcpg_em_totals;
enum { KMCPG_K9_EM = 66 };  /* kmcpg_k4_launch.kernel of K9 */
typedef struct {
  uint64_t reads, none, one, split;              /* k9_em: logged reads; with no / one / several estimated targets */
  uint64_t lds_adds, global_adds, spilled_adds;  /* spilled_adds is part of global_adds */
  uint32_t grid, slots;
  double em_ms;                                  /* HIP-event time at profiling level >= 1; -1 otherwise */
} kmcpg_em_stats;
int kmcpg_em_pass(kmcpg_db* db, const kmcpg_em_class* classes, uint32_t n_classes, uint32_t level_species);
int kmcpg_em_read(kmcpg_db* db, kmcpg_em_col* out_cols, uint32_t n_cols, kmcpg_em_totals* totals);
int kmcpg_last_em(kmcpg_db* db, kmcpg_em_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches);

/* -- the host half of the counting stages (K6, K7, K8) alone: what kmcpg_wait does for the reads of a batch their kernels LEFT, on a list
 *    the caller brings, in K3's hand-over form (pairs grouped by read, segments up to 4096 pairs in final order; read_offs: n_reads + 1
 *    words).  The host's own tests run first (params, -f among them), a longer segment is put in final order here, and each read's final
 *    rows go to the host state of the stages that are on — the counters kmcpg_refstats_read adds, the map kmcpg_cooccur_read merges, the
 *    log kmcpg_recount_run replays.  left_refstats / left_cooccur / left_recount: a byte per read, != 0 = the stage takes the read; NULL =
 *    every read; ignored for a stage that is off.  Needs no GPU (a metadata-only handle will do).  With every stage off: 0, nothing
 *    changes.  KMCPG_EINVAL: read_offs[0] != 0, offsets that run backwards or past read_offs[n_reads], a column the handle does not have
 *    (reads in front of the bad one have been counted: reset the stages). */
int kmcpg_count_left_reads(kmcpg_db* db, const kmcpg_pair* pairs, const uint64_t* read_offs, const int32_t* qkmers, const int32_t* qlen,
                           uint32_t n_reads, const kmcpg_params* params, const uint8_t* left_refstats, const uint8_t* left_cooccur,
                           const uint8_t* left_recount);

/* -- statistics-only search (K10, k10_left.hip): reads in, the counting stages' state on the handle out — no matches come to the host
 *    and nothing is there to be written.  kmcpg_submit_stats takes kmcpg_submit's arguments on a handle with at least one counting stage
 *    on (kmcpg_set_refstats, kmcpg_set_cooccur, kmcpg_set_recount; KMCPG_EINVAL with none) and runs K10 as the batch's last kernels: the
 *    bytes the stages wrote for the reads they LEFT become one mask byte per read (bit 0: K6, bit 1: K7, bit 2: K8), and the segments of
 *    those reads, and only those, are compacted into the batch's dead hit buffer.  Per ticket the two hit counters, K3's last two words,
 *    qlen / qkmers (4 + 4 bytes per read), the mask bytes and the witness words leave the GPU, and — only if a read was LEFT — the
 *    n_reads + 1 offsets of the compacted segments and 8 bytes per LEFT pair: bytes_d2h <= 9 n + 256 without a LEFT read,
 *    <= 17 n + 256 + 8 left_pairs with one.  kmcpg_wait_stats does for the batch what kmcpg_wait does (a batch whose hit buffer overflowed
 *    runs again and is counted once; a batch that fails after it was counted taints the stages) and hands the compacted pairs to the
 *    host half; what kmcpg_refstats_read, kmcpg_cooccur_read, kmcpg_recount_run / _read and kmcpg_em_pass / _read report afterwards is
 *    byte for byte what they report after kmcpg_submit + kmcpg_wait of the same reads.
 *    KMCPG_EINVAL with the species-specific stage on (K4 filters an output this ticket does not have); KMCPG_EUNSUPPORTED on database
 *    sets, on paged / multi-device / sharded handles, with KMCPG_DEVICE_FINALIZE=0, and for the parameters the stages refuse (try_se,
 *    top_n_scores != 0, several k-mer sizes with k == 0).  The ticket is consumed by kmcpg_wait_stats ONLY: kmcpg_wait, kmcpg_wait_pairs
 *    and kmcpg_wait_summaries refuse it (KMCPG_EINVAL, the ticket stays valid), and kmcpg_wait_stats refuses every other ticket.
 *    kmcpg_left_compact_device runs K10 alone on device pointers: K3's output (d_pairs, d_read_offs: n_reads + 1 words, at most pair_cap
 *    pairs), the three stages' bytes (NULL: the stage is not looked at), the overflow guard of the counting kernels (d_n_hits NULL: none;
 *    *d_n_hits > hit_cap: d_mask, d_left_pairs and d_left_offs keep what they held) -> d_mask[n_reads], the LEFT reads' pairs in
 *    d_left_pairs[d_left_offs[i] .. d_left_offs[i + 1]) in their order (d_left_offs: n_reads + 1 words; left_cap >= pair_cap).  It needs
 *    no stage on.  Only enqueues on `stream`.
 *    kmcpg_last_stats: the witness of the handle's last K10 launch (the call waits for the device to go idle) or, after
 *    kmcpg_wait_stats, of that ticket; at profiling level >= 1 the HIP-event time of the handle's last K10 launch and one record per
 *    kernel launched (the scan's records carry KMCPG_K4_SCAN_*). */
enum { KMCPG_K10_MASK = 67, KMCPG_K10_COMPACT = 68, KMCPG_K10_OFFS = 69 };  /* kmcpg_k4_launch.kernel of K10's own kernels */
typedef struct {
  uint64_t n_reads;
  uint64_t matched_reads;  /* reads with at least one pair in K3's output */
  uint64_t kept_pairs;     /* K3's total */
  uint64_t left_reads;     /* reads a counting stage left to the host half */
  uint64_t left_pairs;     /* their pairs: all that came to the host of the batch's matches */
  uint64_t bytes_d2h;      /* bytes that came from the device for the ticket */
} kmcpg_result_stats;
typedef struct {
  uint64_t n_reads, matched_reads, kept_pairs, left_reads, left_pairs;  /* n_reads and kept_pairs: 0 after kmcpg_left_compact_device */
  uint64_t bytes_d2h;      /* 0 after kmcpg_left_compact_device */
  uint64_t bad_segments;   /* segments that did not lie inside pair_cap (treated as empty; must be 0) */
  uint64_t skipped;        /* 1: the overflow guard skipped the launch */
  double k10_ms;           /* HIP-event time of the stage's kernels at profiling level >= 1; -1 otherwise */
} kmcpg_stats_ticket_stats;
int kmcpg_left_compact_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, uint32_t n_reads,
                              const uint8_t* d_left_refstats, const uint8_t* d_left_cooccur, const uint8_t* d_left_recount,
                              const uint64_t* d_n_hits, uint64_t hit_cap, uint8_t* d_mask, kmcpg_pair* d_left_pairs, uint64_t left_cap,
                              uint64_t* d_left_offs, void* stream);
int kmcpg_submit_stats(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const uint8_t* seqs2, const uint64_t* offs2, uint32_t n_reads,
                       const kmcpg_params* params, kmcpg_ticket** out);
int kmcpg_wait_stats(kmcpg_ticket* ticket, kmcpg_result_stats* out);
int kmcpg_last_stats(kmcpg_db* db, kmcpg_stats_ticket_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches);

/* -- taxonomic binning (K11, k11_bin.hip): one TaxId per read — that of the one whitelisted reference it matches, or the lowest common
 *    ancestor of the several (`kmcp profile -B`; the rule and the plan: kmcp_amd/csrc/bin_rule.hpp).
 *    kmcpg_set_binning uploads copies of a plan: node_of_column[n_cols] = the pre-order number, in the plan's pruned tree, of the column's
 *    target, or KMCPG_BIN_NO_NODE where the target is not whitelisted; parent / last / taxid [n_nodes] = the tree (node 0: the virtual
 *    root, parent[0] = 0, last[0] = n_nodes - 1; parent[v] < v <= last[v] <= last[parent[v]] for every other node — KMCPG_EINVAL
 *    otherwise, for a node_of_column that is neither a node nor KMCPG_BIN_NO_NODE, and for a taxid that is KMCPG_BIN_NONE or KMCPG_BIN_LEFT).  (NULL, 0, ...) switches the stage off.  It is
 *    independent of the other stages and refuses the handles kmcpg_set_refstats refuses.
 *    kmcpg_bin_device runs K11 alone on device pointers: K3's output (d_pairs, d_read_offs: n_reads + 1 words, at most pair_cap pairs),
 *    d_qkmers and final_n as for kmcpg_specific_device (a read with pairs and more than final_n k-mers is LEFT: exactly the reads K4
 *    leaves), the overflow guard of the counting stages (d_n_hits NULL: none; *d_n_hits > hit_cap: d_bins keeps what it held)
 *    -> d_bins[n_reads]: the TaxId, KMCPG_BIN_NONE (no whitelisted match: no line) or KMCPG_BIN_LEFT.  Only enqueues on `stream`.
 *    (Its arguments are kmcpg_refstats_device's with d_bins in the place of d_left, not kmcpg_specific_device's plus d_bins: K4's output
 *    arguments — the compacted pairs, their offsets, the verdict bytes — have no counterpart here, and the overflow guard needs the
 *    batch's hit counter.)
 *    kmcpg_last_bins: the witness of the handle's last K11 launch (the call waits for the device to go idle); at profiling level >= 1
 *    the HIP-event time and one record per kernel launched. */
enum { KMCPG_K11_BIN = 70 };  /* kmcpg_k4_launch.kernel of K11's kernel */
#define KMCPG_BIN_NO_NODE 0xffffffffu
#define KMCPG_BIN_NONE 0xffffffffu
#define KMCPG_BIN_LEFT 0xfffffffeu
typedef struct {
  uint64_t no_bin;        /* reads without a whitelisted match (KMCPG_BIN_NONE) */
  uint64_t one;           /* reads whose whitelisted matches name one node of the plan */
  uint64_t several;       /* ... several: the bin is their lowest common ancestor */
  uint64_t left;          /* reads LEFT to the host (KMCPG_BIN_LEFT) */
  uint64_t climb_steps;   /* parent steps of all climbs */
  uint64_t bad_segments;  /* segments that did not lie inside pair_cap (treated as empty; must be 0) */
  uint64_t skipped;       /* 1: the overflow guard skipped the launch */
  uint32_t grid;          /* workgroups launched */
  uint32_t in_lds;        /* 1: the plan's tables were in LDS */
  double k11_ms;          /* HIP-event time of the kernel at profiling level >= 1; -1 otherwise */
} kmcpg_bin_stats;
int kmcpg_set_binning(kmcpg_db* db, const uint32_t* node_of_column, uint32_t n_cols, const uint32_t* parent, const uint32_t* last,
                      const uint32_t* taxid, uint32_t n_nodes);
int kmcpg_bin_device(kmcpg_db* db, const kmcpg_pair* d_pairs, const uint64_t* d_read_offs, uint64_t pair_cap, const int32_t* d_qkmers,
                     uint32_t n_reads, int32_t final_n, const uint64_t* d_n_hits, uint64_t hit_cap, uint32_t* d_bins, void* stream);
int kmcpg_last_bins(kmcpg_db* db, kmcpg_bin_stats* out, kmcpg_k4_launch* launches, uint32_t cap, uint32_t* n_launches);
/*    kmcpg_submit_bins takes kmcpg_submit's arguments on a handle with the stage on (KMCPG_EINVAL with it off); the batch runs K1, K2, K3
 *    and K11 — no other stage behind K3, whatever is on.  kmcpg_wait_bins writes one word per read to bins[n_reads]: the TaxId or
 *    KMCPG_BIN_NONE, never KMCPG_BIN_LEFT.  With no LEFT read only the bins, the two hit counters, K3's last two words and the witness
 *    words leave the GPU: bytes_d2h <= 4 n + 256.  With one, K10's compaction (kmcpg_left_compact_device, K11's LEFT byte as the stage's)
 *    brings the LEFT reads' pairs together, and qkmers (4 bytes per read), the n + 1 offsets and 8 bytes per LEFT pair come down as well:
 *    bytes_d2h <= 16 n + 264 + 8 left_pairs; the host half applies its own -f test to those pairs and then bin_rule.hpp.  A batch whose
 *    hit buffer overflowed runs again — the attempt that overflowed wrote no bin (K11's and K10's guard) — and `reruns` says how often.  Refusals as for kmcpg_submit_stats: KMCPG_EINVAL with the species-specific stage on;
 *    KMCPG_EUNSUPPORTED on database sets, on paged / multi-device / sharded handles, with KMCPG_DEVICE_FINALIZE=0 and for try_se,
 *    top_n_scores != 0 and several k-mer sizes with k == 0.  The ticket is consumed by kmcpg_wait_bins ONLY: the other waits refuse it
 *    (KMCPG_EINVAL, the ticket stays valid), and kmcpg_wait_bins refuses every other ticket.  After kmcpg_wait_bins, kmcpg_last_bins
 *    reports that ticket's counters (`left`: the reads the device LEFT, all binned by the host half since). */
typedef struct {
  uint64_t n_reads;
  uint64_t binned_reads;  /* reads with a TaxId in bins[] */
  uint64_t kept_pairs;    /* K3's total */
  uint64_t host_reads;    /* reads K11 LEFT: binned by the host half */
  uint64_t left_pairs;    /* their pairs: all that came to the host of the batch's matches */
  uint64_t bytes_d2h;     /* bytes that came from the device for the ticket, its last attempt's */
  uint64_t reruns;        /* how often the batch ran again because its hit buffer overflowed: the attempt before wrote no bin */
} kmcpg_result_bins;
int kmcpg_submit_bins(kmcpg_db* db, const uint8_t* seqs, const uint64_t* offs, const uint8_t* seqs2, const uint64_t* offs2, uint32_t n_reads,
                      const kmcpg_params* params, kmcpg_ticket** out);
int kmcpg_wait_bins(kmcpg_ticket* ticket, uint32_t* bins, kmcpg_result_bins* out);

/* -- benchmarking / full-size parity support (no counterpart in the reference) ------------------ */
typedef struct {
  int32_t k;            /* 21 */
  int32_t num_hashes;   /* 1 */
  double fpr;           /* 0.3: the fullest column has bit density 1-exp(-1/ratio) = fpr */
  uint32_t n_blocks;    /* e.g. 32 */
  uint32_t cols_per_block; /* e.g. 14976 */
  uint64_t num_sigs;    /* rows per block, e.g. 970000 */
  uint64_t kmers_per_col; /* Sizes[] of every column, e.g. 346000 */
  uint64_t seed;
  uint32_t scale;       /* 0/1 = all k-mers; >1 = FracMinHash database (`scaled: true`, `scale`) */
  uint32_t syncmer_s;   /* >0 = Closed-Syncmer database */
  uint32_t minimizer_w; /* >0 = Minimizer database */
  uint32_t sigs_step;   /* block i has num_sigs + i*sigs_step rows.  Real databases have a different NumSigs in (almost) every
                           block; blocks with equal NumSigs are laid side by side in HBM and served by one gather */
} kmcpg_synth_spec;
/* Builds a synthetic database directly in HBM: every bit i.i.d. Bernoulli(density) from a
 * counter-based generator keyed by (seed, block, row, word).  Column names are "syn<global col>". */
int kmcpg_open_synthetic(const kmcpg_synth_spec* spec, const kmcpg_opts* opts, kmcpg_db** out);
/* ORs the Bloom bits of the given k-mer hashes into column `col` (global id) if it is local. */
int kmcpg_plant(kmcpg_db* db, uint32_t col, const uint64_t* hashes, uint64_t n);
/* Device-resident variant for whole batches: ORs the Bloom bits of every k-mer of read i (hashed exactly as a
 * query would be) into global column d_cols[i]; 0xFFFFFFFF = do not plant; non-local columns are skipped. */
int kmcpg_plant_reads_device(kmcpg_db* db, const uint8_t* d_seqs, const uint64_t* d_offs, uint32_t n_reads,
                             uint64_t total_bases, uint32_t max_read_len, const uint32_t* d_cols, void* stream);
/* HIP-event timing of the kernels inside kmcpg_query_device (events on the caller's stream).
 * kmcpg_last_timing waits for the last call to finish; times are milliseconds. */
int kmcpg_set_profiling(kmcpg_db* db, int enable);  /* 0 off, 1 timing, 2 timing + count the row loads of the COBS kernel */
/* Bytes the COBS kernel(s) of the last kmcpg_query_device call asked the memory system for (16 B per lane and row actually
 * loaded, row padding included, pruned rows not): a live cross-check of the FETCH_SIZE counter passes.  Level 2 only. */
int kmcpg_last_gathered_bytes(kmcpg_db* db, uint64_t* bytes);
/* ... and the bytes of k-mer hashes the same launches read (8 B per k-mer, once per (read, slot): 0.8 % of the row bytes for
 * 1-KB row tiles, 6 % for 128-byte rows).  Rows + hashes is what FETCH_SIZE sees.  Level 2 only. */
int kmcpg_last_hash_bytes(kmcpg_db* db, uint64_t* bytes);
/* ... and how many waves of those launches finished in tail mode (long queries on 1-KiB row tiles whose sectors had died down
 * to at most four: the idle lanes take shares of the remaining rows, k2_cobs.hip; KMCPG_TAIL_SECTORS=0 switches it off).  Level 2 only. */
int kmcpg_last_tail_waves(kmcpg_db* db, uint64_t* waves);
/* Which COBS kernels the last kmcpg_query_device call launched, one record per launch in launch order (a form launched several
 * times in one call appears as often), written where the kernel is launched from the template parameters of that kernel.  Tests
 * use it to assert which instantiation served a batch.  kind: 0 = k2_cobs, 1 = its chunked long-query form, 2 = k2_cobs_pair
 * (two lane forms in one grid: lpr lanes + lprb lanes).  Profiling level >= 1; the log is cleared at the start of every call. */
typedef struct {
  int32_t kind;
  int32_t lpr;        /* lanes per row tile: 4, 8, 16, 32, 64 */
  int32_t lprb;       /* kind 2: lanes of the second form; otherwise 0 */
  int32_t npl;        /* counter planes: 8, 10, 16, 24 */
  int32_t multi;      /* 1 = the several-hash-functions form */
  int32_t group_rows; /* rows between two pruning tests: 8 or 4 */
  uint32_t workgroups; /* of the launch piece: one wave per unit (lpr 64), four waves per workgroup */
  uint32_t grid;       /* workgroups the kernel was launched on: = workgroups, except for the persistent short-read kernel
                        * (k2_cobs_persist, KMCPG_K2_PERSIST), whose resident waves share the piece's units: the only field that tells it from
                        * the launched form.  kind 2: both halves together */
} kmcpg_k2_launch;
/* Copies up to `cap` records to out (may be NULL when cap is 0); *n = how many launches the call made. */
int kmcpg_last_k2_launches(kmcpg_db* db, kmcpg_k2_launch* out, uint32_t cap, uint32_t* n);
int kmcpg_last_timing(kmcpg_db* db, float* kmers_ms, float* cobs_ms);
/* The same for an earlier call: age 0 = the last one, 1 = the one before ... (the last 4 are kept), so that a caller with
 * several batches in flight can read the times of a finished one without waiting for the newest. */
int kmcpg_timing_at(kmcpg_db* db, uint32_t age, float* kmers_ms, float* cobs_ms);
/* Copies rows (on-disk width NumRowBytes each) of a local block back to the host. */
int kmcpg_read_rows(kmcpg_db* db, uint32_t block, const uint64_t* row_idx, uint64_t n_rows, uint8_t* out);
/* The same for rows first_row .. first_row + n_rows - 1 (bench: the index goes back to the host for the CPU baseline). */
int kmcpg_read_row_range(kmcpg_db* db, uint32_t block, uint64_t first_row, uint64_t n_rows, uint8_t* out);
/* Geometry of block b (global index): NumSigs, columns, NumRowBytes, device row stride, is-local. */
int kmcpg_block_info(const kmcpg_db* db, uint32_t block, uint64_t* num_sigs, uint32_t* n_cols, uint32_t* row_bytes,
                     uint32_t* dev_stride, int32_t* is_local, uint32_t* col_base);
/* k-mer generation only (K1): returns hashes of read i at d_hashes[d_koff[i] .. +d_nk[i]). Debug/tests. */
int kmcpg_kmers_device(kmcpg_db* db, const uint8_t* d_seqs, const uint64_t* d_offs, uint32_t n_reads,
                       uint64_t total_bases, uint32_t max_read_len, const kmcpg_params* params,
                       uint64_t* d_hashes, uint64_t hashes_cap, uint64_t* d_koff, int32_t* d_nk, void* stream);
/* The same on a batch that is on the device as 2-bit codes (the layout of kmcpg_submit_packed: base j of the batch in bits 2 (j % 4)
 * of d_codes[j / 4], 16 readable bytes behind the last one, 4-byte aligned; d_exc = its n_exc runs of foreign bytes on the device)
 * and d_text = total_bases + 16 writable bytes for whatever has to be expanded: whole genomes (k <= 128, plain or FracMinHash k-mers)
 * are hashed from the codes directly and only the 65 536-position segments a foreign byte reaches become text (k1_seg.hip);
 * every other shape of batch is expanded whole first.  Debug/tests. */
int kmcpg_kmers_device_packed(kmcpg_db* db, const uint8_t* d_codes, const kmcpg_exc_run* d_exc, uint32_t n_exc, uint8_t* d_text,
                              const uint64_t* d_offs, uint32_t n_reads, uint64_t total_bases, uint32_t max_read_len,
                              const kmcpg_params* params, uint64_t* d_hashes, uint64_t hashes_cap, uint64_t* d_koff, int32_t* d_nk,
                              void* stream);
/* The same for paired reads: mates in d_seqs2 / d_offs2 (both required), total_bases and hashes_cap over BOTH mates, max_read_len the
 * longest single mate.  The hashes of pair i — mate 1's list, then mate 2's — start at d_hashes[d_offs[i] + d_offs2[i]], d_nk[i] of them,
 * as on the query path; d_nk1 (optional, n_reads words) receives the first mate's raw count, what --try-se relies on.  Debug/tests. */
int kmcpg_kmers_device_paired(kmcpg_db* db, const uint8_t* d_seqs, const uint64_t* d_offs, const uint8_t* d_seqs2, const uint64_t* d_offs2,
                              uint32_t n_reads, uint64_t total_bases, uint32_t max_read_len, const kmcpg_params* params,
                              uint64_t* d_hashes, uint64_t hashes_cap, int32_t* d_nk, int32_t* d_nk1, void* stream);
/* The same on a staged piece of sliding windows (kmcpg_submit_windows), exactly as a lane runs it: the piece's descriptors are built on
 * the device (k_window_desc, windows.hip), then the k-mer stage (K1 + dedup) reads every window's bases in place.  All pointers are
 * device memory.  d_text = the staged slices of reads one behind the other, staged_bases of them, with 16 readable bytes behind the last
 * (the lane's own allowance); d_soffs / d_wpre / d_vpre / d_cpre = n_slices + 1 words each: the prefix sums over the slices of their
 * bases, their windows, their windows' bases and their chunks of 1 024 k-mer positions (0 for a slice shorter than k), as
 * kmcp_amd/csrc/window_plan.hpp stage_windows states them; n_chunks = d_cpre[n_slices], n_windows = d_wpre[n_slices], window_bases =
 * d_vpre[n_slices], max_window_len = the longest window.  Out: d_koff[n_windows + 1] = where each window's list starts in d_hashes
 * (the prefix of window bases; hashes_cap >= window_bases), d_src[n_windows] = each window's first base in d_text, d_nk[n_windows] =
 * NumKmers, d_qlen[n_windows] = the window's length.  No window (n_windows = 0): nothing is launched.  KMCPG_EINVAL: a null pointer, a
 * spec that kmcpg_submit_windows refuses, sizes that contradict each other, hashes_cap too small.  Debug/tests. */
int kmcpg_kmers_device_windows(kmcpg_db* db, const uint8_t* d_text, const uint64_t* d_soffs, const uint64_t* d_wpre, const uint64_t* d_vpre,
                               const uint64_t* d_cpre, uint32_t n_slices, uint64_t staged_bases, uint64_t n_chunks, uint32_t n_windows,
                               uint64_t window_bases, uint32_t max_window_len, const kmcpg_window_spec* spec, const kmcpg_params* params,
                               uint64_t* d_hashes, uint64_t hashes_cap, uint64_t* d_koff, uint64_t* d_src, int32_t* d_nk, int32_t* d_qlen,
                               void* stream);
/* Which k-mer kernels (K1, k1_kmers.hip) the handle's last k-mer stage launched — kmcpg_kmers_device*, kmcpg_query_device, a submit,
 * kmcpg_plant_reads_device — one record per launch in launch order, written where the kernel is launched from the template
 * parameters of the function that launches it.  The first record (kernel KMCPG_K1_PLAN) is the plan of the call (k1_plan.hpp): p0 =
 * the form (KMCPG_K1F_*), p1 = bit 0 codes_direct, bit 1 list_fallback, bit 2 adj_done, left_on_list = for the two list forms
 * (SegRoll2, WindowsRoll) how many segments / reads the first kernel left to the fallback kernel behind it, read back by the
 * kmcpg_kmers_device* entries only; UINT32_MAX = not read (every other entry point: nothing is synchronised for it) or no list.
 * Recorded at profiling level >= 1 only: *n = 0 otherwise, and nothing is added to the stream.  Cleared by every k-mer stage. */
enum {
  KMCPG_K1_PLAN = 0,
  KMCPG_K1_KMERS,         /* k1_kmers<p0 = MODE> */
  KMCPG_K1_KMERS_WG,      /* k1_kmers_wg<p0 = MODE> */
  KMCPG_K1_KMERS_WG_GLOBAL,
  KMCPG_K1_WINDOWS_WAVE,  /* k1_windows_wave<p0 = MODE> */
  KMCPG_K1_WINDOWS_ROLL,  /* k1_windows_roll<p0 = WSZ, p1 = WAVES> */
  KMCPG_K1_SEG_ROLL2,
  KMCPG_K1_SEG_ROLL,
  KMCPG_K1_SEG_HASH,
  KMCPG_K1_SEG_PACK,
  KMCPG_K1_MARK_EXC,
  KMCPG_K1_UNPACK2_LIST,
  KMCPG_K1_WIN_HASH,
  KMCPG_K1_WIN_SCAN,
  KMCPG_K1_WIN_RANK,
  KMCPG_K1_WIN_GATHER,
  KMCPG_K1_KERNELS
};
enum { KMCPG_K1F_NONE = 0, KMCPG_K1F_WIN_ONCE, KMCPG_K1F_SEG_ROLL2, KMCPG_K1F_SEG_ROLL, KMCPG_K1F_SEG_HASH, KMCPG_K1F_WINDOWS_ROLL,
       KMCPG_K1F_WINDOWS_WAVE, KMCPG_K1F_WG_GLOBAL, KMCPG_K1F_WG, KMCPG_K1F_SHORT };
typedef struct {
  int32_t kernel;        /* KMCPG_K1_* */
  int32_t p0, p1;        /* template parameters of the kernel (0 where it has none); the plan record: see above */
  uint32_t grid, block;  /* workgroups, threads per workgroup */
  uint32_t lds_bytes;    /* dynamic LDS of the launch */
  uint32_t left_on_list; /* the plan record only; UINT32_MAX elsewhere */
  uint32_t reserved;
} kmcpg_k1_launch;
/* Copies up to `cap` records to out (may be NULL when cap is 0); *n = how many there are. */
int kmcpg_last_k1_launches(kmcpg_db* db, kmcpg_k1_launch* out, uint32_t cap, uint32_t* n);
typedef struct kmcpg_sketch_launch kmcpg_sketch_launch; /* defined with kmcpg_sketch_genomes below */
/* The segmented sort + unique of kmcpg_sketch_genomes (sort_segments.hip) on lists the caller lays out; needs no handle and runs on
 * the current device.  Debug/tests.  All pointers but rec are device memory.  List s is the concatenation over parts p < parts of
 * d_keys[p * part_stride + d_in_off[s] .. + d_cnt[p * cnt_stride + s]); every list lies inside its part, d_keys holds
 * part_stride * parts words and is left intact (the sort runs on a copy, in the buffer arrangement of kmcpg_sketch_genomes).
 * key_bits: no key has a bit set at or above it; max_waves: at least the sum over the lists of ceil(keys / 4096).  On return (the
 * stream synchronised) list s is d_out[d_koff[s] .. d_koff[s + 1]), ascending and unique; d_koff has n_segs + 2 words, the last
 * one holds the number of raw keys.  out_cap (words of d_out) must be at least part_stride * parts, whatever the lists hold.  rec
 * (host, may be NULL) receives the launch record.  KMCPG_EINVAL before anything is launched: a null pointer, parts outside 1..8,
 * key_bits outside 0..64, cnt_stride < n_segs, part_stride >= 2^32, out_cap too small; from the sizes read back: a negative count,
 * a list outside its part, 2^32 raw keys or more, more raw keys than part_stride * parts (lists that overlap), more waves than
 * max_waves; and what the sort's launcher itself refuses: key_bits == 0 with max_waves > 0. */
int kmcpg_sort_segments_device(const uint64_t* d_keys, const uint64_t* d_in_off, const int32_t* d_cnt, uint64_t part_stride,
                               uint32_t cnt_stride, int32_t parts, uint32_t n_segs, uint32_t max_waves, int32_t key_bits,
                               uint64_t* d_out, uint64_t out_cap, uint64_t* d_koff, kmcpg_sketch_launch* rec, void* stream);
typedef struct { int32_t dedup_threshold, min_matched, pre, pre_done, key_shift; } kmcpg_dedup_spec;
/* debug/tests: the dedup stage of the k-mer step alone, on hash lists laid out in device memory by the caller.  Query r's list is
 * d_hashes[d_offs[r] (+ d_offs2[r]) ...], d_nk_raw[r] long; max_n >= every d_nk_raw[r]; d_scratch is as large as d_hashes.
 * Above dedup_threshold (-u) a list is sorted and made unique in place and d_nk_search[r] is its new length, at or below it the list
 * stays as it is and d_nk_search[r] = d_nk_raw[r]; either is 0 where d_nk_raw[r] < min_matched.  pre: adjacent repeats are dropped
 * first (window sketches), into d_scratch; pre_done: the caller has done that already, for the queries with a raw count in
 * (max(dedup_threshold, 512), 65536]: their shortened lists are in d_scratch and the lengths in d_nk_search.  key_shift: leading zero
 * bits of the largest possible key (0, or clz(maxHash) of a FracMinHash database): no key may have a bit set above it.  Slots must
 * not overlap.  Enqueues on `stream`; a batch with a query above 65 536 keys synchronises it on the way (the handle's workspace
 * holds the device-wide sort's tables).  KMCPG_DEDUP_BIG_BUCKET is read at every call. */
int kmcpg_dedup_device(kmcpg_db* db, uint64_t* d_hashes, uint64_t* d_scratch, const uint64_t* d_offs, const uint64_t* d_offs2,
                       const int32_t* d_nk_raw, int32_t* d_nk_search, uint32_t n_reads, uint64_t max_n,
                       const kmcpg_dedup_spec* spec, void* stream);
/* Which kernels the handle's last dedup stage launched (k1_dedup.hip, sort_huge.hip) — the one inside kmcpg_kmers_device*,
 * kmcpg_query_device, a submit, kmcpg_plant_reads_device, or kmcpg_dedup_device — one record per launch in launch order, written where
 * the kernel is launched.  The first record names the branch the stage took: KMCPG_DD_LAUNCH_DEDUP (some query may be above -u; no
 * kernel of its own; its p0, p1, p2 = how many queries the k_dedup_bucket launches of 2048, 4096 and 16384 elements sent to their bitonic
 * fallback, read from the device when this is called: synchronise the stage's stream first) or KMCPG_DD_NK_SIMPLE (k_nk_simple alone).  In
 * every other record p0..p2 are the template parameters of the instantiation (CAP, NB, NT
 * of k_dedup_bucket; NT, CAP of k_dedup), lo / hi the class of elements to sort the launch takes (lo < m <= hi).  The kernels of the
 * device-wide sort of one query above 65 536 keys: lo = the query, hi = its raw count, p0 = the bit the radix pass starts at (k_rs_*).
 * Recorded at profiling level >= 1 only: *n = 0 otherwise.  Cleared by every dedup stage. */
enum {
  KMCPG_DD_LAUNCH_DEDUP = 0,
  KMCPG_DD_NK_SIMPLE,
  KMCPG_DD_WAVE,          /* k_dedup_wave */
  KMCPG_DD_ADJ_UNIQUE,    /* k_adj_unique */
  KMCPG_DD_BUCKET,        /* k_dedup_bucket<p0 = CAP, p1 = NB, p2 = NT> */
  KMCPG_DD_WG,            /* k_dedup<p0 = NT, p1 = CAP> */
  KMCPG_DD_RS_HIST,
  KMCPG_DD_SCAN_TILE_SUMS,
  KMCPG_DD_SCAN_U32,
  KMCPG_DD_SCAN_TILES,
  KMCPG_DD_RS_SCATTER,
  KMCPG_DD_UQ_COUNT,
  KMCPG_DD_UQ_SCATTER,
  KMCPG_DD_SET_NK_HUGE,
  KMCPG_DD_KERNELS
};
typedef struct {
  int32_t kernel;        /* KMCPG_DD_* */
  int32_t p0, p1, p2;    /* see above; 0 where the kernel has none */
  uint32_t grid, block;  /* workgroups, threads per workgroup (0 for KMCPG_DD_LAUNCH_DEDUP and KMCPG_DD_NK_SIMPLE: the branch) */
  int32_t lo, hi;
} kmcpg_dedup_launch;
/* Copies up to `cap` records to out (may be NULL when cap is 0); *n = how many there are. */
int kmcpg_last_dedup_launches(kmcpg_db* db, kmcpg_dedup_launch* out, uint32_t cap, uint32_t* n);
/* Batches of this handle so far whose k-mer kernels read 2-bit codes directly (packed whole-genome batches), and packed batches that
 * were expanded to text first. */
int kmcpg_k1_codes_batches(kmcpg_db* db, uint64_t* direct, uint64_t* expanded);

/* -- index inspection: what `kmcp utils index-density` counts (kmcp/cmd/index-density.go:139-213) and the measured side of
 *    `kmcp utils ref-info` (ref-info.go:128-150), from resident rows.  Read-only; every number is an integer a caller can recount from
 *    the file.  The rows of block `block` from first_row on (n_rows of them, 0 = to the block's last row) are cut into bins of bin_rows
 *    rows — the last bin may be short — and kmcpg_block_density counts the set bits of every column in every bin.  The calls take the
 *    handle's enqueue lock as the GPU half of a search does, allocate their device scratch per call and free it before they return
 *    (KMCPG_ENOMEM names the bytes asked for); they may be used beside kmcpg_submit / kmcpg_wait on a kmcpg_open handle.
 *    KMCPG_EINVAL: non-local block, bin_rows == 0, rows outside the block, cap too small, reserved != 0.  KMCPG_EUNSUPPORTED: paged
 *    (kmcpg_open_paged) and multi-device (kmcpg_open_devices) front handles.  KMCPG_EDEVICE: metadata-only handles. */
typedef struct {
  uint64_t bin_rows;   /* >= 1 */
  uint64_t first_row;  /* 0 */
  uint64_t n_rows;     /* 0 = to the block's last row */
  uint64_t reserved;   /* must be 0 */
} kmcpg_density_spec;
/* n_bins = ceil(rows / bin_rows): the last bin may be short */
int kmcpg_density_bins(const kmcpg_db* db, uint32_t block, const kmcpg_density_spec* spec, uint64_t* n_bins);
/* counts[c * n_bins + b], c = column of the block (host memory, cap in elements) */
int kmcpg_block_density(kmcpg_db* db, uint32_t block, const kmcpg_density_spec* spec, uint32_t* counts, uint64_t cap);
/* set bits of every global column over all its rows; 0 for columns of non-local blocks.  One pass over every resident group. */
int kmcpg_col_ones(kmcpg_db* db, uint64_t* ones, uint64_t cap);
/* what the last density call launched: form (0 carry-save planes, 1 small-bin bit extracts), lanes per row tile and planes (form 0; of the
 * last launch), workgroups of the form-0 launches together, launches */
typedef struct {
  int32_t form, lpr, npl, reserved;
  uint32_t workgroups, launches;
} kmcpg_density_launch;
int kmcpg_last_density_launch(kmcpg_db* db, kmcpg_density_launch* out);
/* A handle over the given .uniki files alone, no __db.yml needed: headers parsed and checked for mutual compatibility as kmcpg_open
 * checks them (serialization.go:90-99), rows resident when device >= 0 (-1: metadata only), blocks numbered in argument order, every
 * block local.  Inspecting one block of a large database uploads only that block.  Work: the inspection calls above, kmcpg_db_info,
 * kmcpg_block_info, kmcpg_col_info, kmcpg_read_rows, kmcpg_read_row_range.  Every search entry point refuses with KMCPG_EUNSUPPORTED
 * (the handle knows neither the database's fpr nor how its k-mers were sketched). */
int kmcpg_open_files(const char* const* uniki_paths, uint32_t n, int32_t device, kmcpg_db** out);

/* bench support (tools/bench_density.py): HIP-event milliseconds of the device work of the last kmcpg_block_density / kmcpg_col_ones call
 * (memsets and kernels, before the copy to the host), and a yardstick for it — kmcpg_stream_probe reads the rows of every resident
 * group once with 16 B per lane and one XOR per load (one launch per group, as kmcpg_col_ones) and reports its HIP-event time and bytes. */
int kmcpg_last_density_ms(kmcpg_db* db, float* ms);
int kmcpg_stream_probe(kmcpg_db* db, float* ms, uint64_t* bytes);

/* -- index building on the GPU ("next" row of SURVEY.md §8f): the Bloom-column scatter of `kmcp index`
 *    (kmcp/cmd/index.go:657-682 block layout, :1023 signature size, :1107-1309 scatter, index/serialization.go:159-300 file,
 *    util-db-info.go:46-79 __db.yml) from lists of k-mer hashes — what the .unik files of `kmcp compute` hold.  Writes
 *    <out_dir>/R001/{_blockNNN.uniki, __db.yml, __name_mapping.tsv} byte-compatible with the reference's reader.  The block
 *    layout includes the big-genome rules (index.go:787-894: smaller blocks above -x/-8, single-column blocks above -1). */
typedef struct {
  int32_t k;
  int32_t canonical;
  int32_t num_hashes;   /* -n */
  double fpr;           /* -f */
  int32_t threads;      /* -j: block size = (int(#cols/threads)+7)/8*8 clamped to [8, #cols] when block_size == 0 */
  int32_t block_size;   /* -b */
  uint32_t scale;       /* recorded in __db.yml (scaled: scale > 1) */
  uint32_t minimizer_w;
  uint32_t syncmer_s;
  int32_t split_seq, split_size, split_num, split_overlap; /* recorded in __db.yml */
  const char* alias;
  /* big-genome block rules, flags -x / -X / -8 / -1 of `kmcp index` (index.go:1453-1463); 0 = the reference's default */
  uint64_t kmers_x;     /* -x 10M (M = 2^20): columns with more k-mers go to blocks of block_size_x columns */
  int32_t block_size_x; /* -X 256 */
  int32_t uniform_sigs; /* 0 = NumSigs per block as `kmcp index` sizes it (index.go:936-946, :1023: files byte-identical to the
                           reference's).  Not in the reference: 1 = every block of a size tier gets the tier's largest NumSigs,
                           2 = NumSigs rounded up to a 5/4 ladder (< 25 % larger files).  Blocks with equal NumSigs are served
                           by ONE gather when resident (grouped rows): a `-j 32` index of 39-byte rows runs at the speed of
                           1248-byte rows.  A larger filter only lowers a block's FPR; any kmcp reader accepts the files. */
  uint64_t kmers_8;     /* -8 20M: ... to blocks of 8 columns */
  uint64_t kmers_1;     /* -1 200M: ... to a block of their own */
} kmcpg_build_cfg;
typedef struct {
  const char* name;       /* reference name */
  uint64_t gsize;         /* genome size */
  uint32_t chunk_idx;     /* index of this chunk */
  uint32_t chunks;        /* number of chunks of the genome */
  const uint64_t* hashes; /* host pointer: sorted-unique k-mer hashes of the chunk */
  uint64_t n_hashes;
} kmcpg_build_col;
int kmcpg_build_db(const char* out_dir, const kmcpg_build_cfg* cfg, const kmcpg_build_col* cols, uint32_t n_cols, int32_t device);
/* The resident database written back as <out_dir>/R001/{_blockNNN.uniki, __db.yml, __name_mapping.tsv} in the reference's format
 * (index/serialization.go:159-300, util-db-info.go:46-79): bench.py puts its synthetic configs[1] index (planted reads included) on
 * /dev/shm this way and searches it with kmcp-search, FASTQ in, TSV out.  Every block must be resident on the handle. */
int kmcpg_save_db(kmcpg_db* db, const char* out_dir);

/* -- sketching reference genomes: `kmcp compute` in --split-number mode (kmcp/cmd/compute.go:569-826) without a database handle —
 *    the records of a file joined, cut into chunks, the k-mers of every chunk hashed (the K1 kernels of the search path, chosen
 *    through k1_plan.hpp), sorted and de-duplicated (sort_segments.hip: all chunk lists of a batch in one set of launches).  The
 *    lists slot straight into kmcpg_build_col.  Structs are zeroed, then filled, then validated (as kmcpg_window_spec). */
typedef struct {
  int32_t ks[8];        /* k-mer sizes, 1 <= k <= 64 (compute.go:176-181), the first n_k entries; a chunk's list holds the k-mers of all */
  int32_t n_k;          /* 1 .. 8 */
  uint32_t scale;       /* -D: 0 / 1 = every k-mer, > 1 = FracMinHash (hash <= maxHash) */
  uint32_t minimizer_w; /* -W, 0 = off; not together with syncmer_s */
  uint32_t syncmer_s;   /* -S, 0 = off */
  uint32_t reserved[4]; /* must be 0 */
} kmcpg_sketch_cfg;     /* always canonical (compute.go:752) */
typedef struct {
  uint32_t split_number;  /* -n: 0 / 1 = one chunk per genome */
  uint32_t split_overlap; /* -l */
  uint64_t split_min_ref; /* -m: a shorter genome is one chunk */
  int32_t k_min, k_max;   /* smallest / largest k of the cfg (k_max is what the joiner pads records with, k_min drops short windows) */
  uint64_t reserved;      /* must be 0 */
} kmcpg_split_spec;
typedef struct kmcpg_sketcher kmcpg_sketcher;
typedef struct {
  uint32_t n_chunks;
  uint32_t reserved;
  uint32_t* genome;    /* [n_chunks] index of the genome in the batch */
  uint32_t* chunk_idx; /* [n_chunks] index of the chunk among the genome's surviving chunks */
  uint32_t* chunks;    /* [n_chunks] the genome's number of chunks */
  uint64_t* koff;      /* [n_chunks + 1] list i is hashes[koff[i] .. koff[i + 1]) */
  uint64_t* hashes;    /* ascending, unique; page-locked host memory (as kmcpg_host_alloc gives) */
  void* owner;         /* internal */
} kmcpg_sketch_result;
/* what the segmented sort of the last kmcpg_sketch_genomes call launched, one record per piece of the batch */
struct kmcpg_sketch_launch {
  int32_t kind;        /* 0 = segmented LSD radix sort + unique */
  int32_t passes;      /* 8-bit radix passes: ceil(key_bits / 8) */
  int32_t key_bits;    /* 64, or the bits of maxHash for FracMinHash sketches */
  uint32_t segments;   /* chunk lists */
  uint32_t workgroups; /* of the histogram / scatter launches */
  uint32_t launches;   /* kernels launched: a function of passes alone */
  uint64_t keys;       /* raw k-mer hashes sorted */
};
int kmcpg_sketcher_open(const kmcpg_sketch_cfg* cfg, int32_t device, kmcpg_sketcher** out);
int kmcpg_sketcher_close(kmcpg_sketcher* s);
/* host only: the chunks [first[i], end[i]) of a joined sequence of `len` bases, in order; *n = how many survive (the genome's
 * `chunks`), the first min(*n, cap) are written (split_plan.hpp restates compute.go:675-744) */
int kmcpg_split_bounds(uint64_t len, const kmcpg_split_spec* spec, uint64_t* first, uint64_t* end, uint64_t cap, uint64_t* n);
/* genome g is seqs[offs[g] .. offs[g + 1]) (host text, the records already joined).  Every genome's bases are uploaded once and the
 * k-mer kernels read each chunk in place.  A batch whose chunks do not fit the workspace (KMCPG_SKETCH_PIECE_BASES bases of chunks,
 * default 2^28) is sketched in pieces and answered as one result. */
int kmcpg_sketch_genomes(kmcpg_sketcher* s, const uint8_t* seqs, const uint64_t* offs, uint32_t n_genomes, const kmcpg_split_spec* spec,
                         kmcpg_sketch_result* out);
void kmcpg_sketch_result_free(kmcpg_sketch_result* r);
/* copies up to `cap` records to out (may be NULL when cap is 0); *n = pieces of the last call */
int kmcpg_last_sketch_launches(kmcpg_sketcher* s, kmcpg_sketch_launch* out, uint32_t cap, uint32_t* n);
/* HIP-event milliseconds of the last call's device work: the k-mer kernels, and the segmented sort + unique (bench support) */
int kmcpg_last_sketch_ms(kmcpg_sketcher* s, float* kmers_ms, float* sort_ms);

/* -- sketch lists that stay on the device: kmcpg_sketch_genomes with a sink in place of the copy of the lists to the host.  Per piece
 *    of the batch (see kmcpg_sketch_genomes) the k-mer kernels and the segmented sort run and koff is read back, exactly as there; then
 *    the sink is called with the piece's chunks and the lists in device memory.  Work the sink enqueues on `stream` runs behind the
 *    sort.  After the sink returns the sketcher synchronises its stream before the next piece reuses the buffers, so the sink need not
 *    wait for what it enqueued; d_hashes is NOT valid after that.  A non-zero return of the sink ends the call with that code (the
 *    sketcher stays usable).  A sink that reads koff alone counts the k-mers of every chunk without moving a list.
 *    kmcpg_sketch_genomes itself is this call with an internal sink that copies the lists to page-locked host memory. */
typedef struct {
  uint32_t first_chunk, n_chunks;               /* this piece's chunks within the call */
  const uint32_t *genome, *chunk_idx, *chunks;  /* host, [n_chunks]: as kmcpg_sketch_result */
  const uint64_t* koff;                         /* host, [n_chunks + 1], offsets into d_hashes (koff[0] == 0) */
  const uint64_t* d_hashes;                     /* DEVICE: ascending, unique */
  void* stream;                                 /* hipStream_t: work enqueued here runs behind the sort */
} kmcpg_sketch_piece;
typedef int (*kmcpg_sketch_sink)(void* user, const kmcpg_sketch_piece* piece);
int kmcpg_sketch_genomes_to(kmcpg_sketcher* s, const uint8_t* seqs, const uint64_t* offs, uint32_t n_genomes, const kmcpg_split_spec* spec,
                            kmcpg_sketch_sink sink, void* user);

/* -- building a database larger than host memory: `kmcp index` in two passes over the input (build_plan.hpp, builder.cpp).  The block
 *    layout of `kmcp index` needs every column's k-mer COUNT (the columns are sorted by it before blocks are cut, index.go:667) but not
 *    the lists.  Pass 1 tells the builder the counts (kmcpg_builder_add_cols); kmcpg_builder_plan lays out the blocks exactly as
 *    kmcpg_build_db does (index.go:657-682, :787-894, :1023) and partitions them, in file order, into rounds whose matrices fit
 *    `matrix_budget` bytes of HBM together (a block counts its matrix + 8 bytes; a round closes when the next block would exceed the
 *    budget; a single block above the budget is refused, KMCPG_ENOMEM, with the block, its bytes and the budget).  Pass 2, per round:
 *    kmcpg_builder_begin_round allocates and zeroes the round's matrices, kmcpg_builder_scatter_device ORs device-resident lists (what a
 *    kmcpg_sketch_sink receives) into them — one kernel launch per call, whatever number of lists and blocks (build_scatter.hip) —
 *    and kmcpg_builder_end_round writes the round's _blockNNN.uniki and frees the matrices.  kmcpg_builder_finish writes __db.yml and
 *    __name_mapping.tsv.  The files are byte-identical to kmcpg_build_db's on the same lists (index/serialization.go:159-300,
 *    util-db-info.go:46-79).  Host memory is O(columns); no list crosses PCIe.
 *
 *    Call order: add_cols* -> plan -> per round (any order of rounds) begin_round / scatter_device* / end_round -> finish.  A call out
 *    of order returns KMCPG_EINVAL and says which call was expected; the handle stays usable.  Structs are zeroed, then filled, then
 *    validated (as kmcpg_sketch_cfg).  A builder opened with device -1 plans only: plan (with an explicit budget), col_place and
 *    block_info work, begin_round returns KMCPG_EDEVICE. */
typedef struct kmcpg_builder kmcpg_builder;
typedef struct {
  kmcpg_build_cfg build;  /* as kmcpg_build_db takes it */
  uint64_t hbm_reserve;   /* kmcpg_builder_plan with matrix_budget 0: budget = free HBM at the call - hbm_reserve */
  uint64_t reserved[3];   /* must be 0 */
} kmcpg_builder_cfg;
typedef struct {
  const char* name;    /* reference name (copied) */
  uint64_t gsize;      /* genome size */
  uint32_t chunk_idx;  /* index of this chunk */
  uint32_t chunks;     /* number of chunks of the genome */
  uint64_t n_hashes;   /* k-mers of the chunk: the length of its sorted-unique list */
} kmcpg_build_colmeta;
typedef struct {
  uint32_t rounds_done;
  uint32_t slice_keys;            /* keys of one list a wave of the scatter kernel takes */
  uint64_t scatter_calls;         /* kmcpg_builder_scatter_device calls that passed their checks */
  uint64_t scatter_launches;      /* kernels launched: == the calls that held at least one key of the open round */
  uint64_t keys_scattered;
  uint64_t lists_skipped;         /* lists of columns of other rounds, and entries given as UINT32_MAX */
  uint64_t matrix_bytes_resident; /* now (padding included) */
  uint64_t matrix_bytes_peak;
  double scatter_ms;              /* HIP-event milliseconds of the scatter kernels (waits for those still running) */
  uint64_t reserved[2];
} kmcpg_builder_stats;
int kmcpg_builder_open(const kmcpg_builder_cfg* cfg, int32_t device /* -1: planning only */, kmcpg_builder** out);
/* pass 1; input order = column id.  A column without k-mers is in no block (index.go:799-801) but keeps its line in __name_mapping.tsv */
int kmcpg_builder_add_cols(kmcpg_builder* b, const kmcpg_build_colmeta* cols, uint32_t n);
int kmcpg_builder_plan(kmcpg_builder* b, uint64_t matrix_budget /* 0: free HBM - hbm_reserve */, uint32_t* n_blocks, uint32_t* n_rounds);
/* block UINT32_MAX (col_in_block and round too): an empty column, in no block */
int kmcpg_builder_col_place(const kmcpg_builder* b, uint32_t col, uint32_t* block, uint32_t* col_in_block, uint32_t* round);
int kmcpg_builder_block_info(const kmcpg_builder* b, uint32_t block, uint64_t* num_sigs, uint32_t* n_cols, uint32_t* row_bytes, uint32_t* round);
int kmcpg_builder_begin_round(kmcpg_builder* b, uint32_t round);
/* list i is d_hashes[koff[i] .. koff[i + 1]) (DEVICE memory; koff and cols are HOST arrays) and belongs to column cols[i]; UINT32_MAX
 * = skip the entry.  A list whose column is in a block of another round is skipped silently (lists_skipped).  Refused before anything
 * is launched (KMCPG_EINVAL): a column id out of range, a column given twice in the round, a list whose length differs from the
 * n_hashes of pass 1 (a file that changed between the passes; the column and both counts are named).  The kernel is enqueued on
 * `stream` (hipStream_t); the call does not wait for it, and d_hashes must stay valid until it has run. */
int kmcpg_builder_scatter_device(kmcpg_builder* b, const uint64_t* d_hashes, const uint64_t* koff, const uint32_t* cols, uint32_t n_lists, void* stream);
/* waits for the device, writes <out_dir>/R001/_blockNNN.uniki of the round's blocks (rows through a page-locked buffer in pieces of at
 * most 256 MB) and frees the matrices.  Refuses (KMCPG_EINVAL, nothing written, round still open) while a non-empty column of the round
 * has not been scattered, naming it: a block file never lacks a column. */
int kmcpg_builder_end_round(kmcpg_builder* b, const char* out_dir);
/* __db.yml and __name_mapping.tsv; refuses while a round is open or one was never built */
int kmcpg_builder_finish(kmcpg_builder* b, const char* out_dir);
int kmcpg_builder_info(kmcpg_builder* b, kmcpg_builder_stats* out);
int kmcpg_builder_close(kmcpg_builder* b);

#ifdef __cplusplus
}
#endif
#endif
