// kernels.hpp — host-callable launchers of the HIP kernels in k1_kmers.hip (K1 entry; kernels in k1_reads.hip, k1_windows.hip, k1_seg.hip,
// k1_win_once.hip), k1_dedup.hip, k2_cobs.hip, k3_finalize.hip (K3 and its scan), k4_specific.hip, k5_summary.hip, k6_refstats.hip, k7_cooccur.hip, k8_recount.hip, k9_em.hip, k10_left.hip, k11_bin.hip (the
// stages behind K3; their shared walk is seg_walk.hpp), density.hip, windows.hip, build_scatter.hip, support.hip and sort_huge.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "common.hpp"
#include "density_core.hpp"
#include "k1_plan.hpp"
#include "k2_plan.hpp"

namespace kmcpg {

// What form WinOnce of launch_k1 works on besides K1Args (no other form reads it) — the hash-once form of plain / FracMinHash windows
// (k <= 65, single-end): every k-mer position of the staged slices `w` is hashed once (h[], one wave per K1_WIN_CHUNK positions), the kept
// ones are compacted in order (kept[]) with each position's rank (rank[]), then every window's list is the run
// kept[rank[i] .. rank[e - k + 1]) copied to a.hashes[a.offs[w] ...]; nk_raw / nk1 / qlen as k1_kmers<0> writes them.
// h / kept / rank: K1Plan::win_words (one per staged base), cnt / cbase: K1Plan::win_chunk_words
struct K1WinOnce {
  WindowSrc w;
  uint64_t *h, *kept;
  uint32_t *rank, *cnt;
  uint64_t* cbase;
};
// K1: the kernels of the plan's form (k1_plan.hpp); `a` complete, side buffer pointers included.  Whether adjacent repeats are already
// dropped afterwards is the plan's adj_done
// what launch_k1 notes about every kernel it launches (kmcpg_last_k1_launches): written at the launch site from the template parameters
// of the launching function.  nullptr = no log (and nothing else differs)
typedef std::vector<kmcpg_k1_launch> K1Log;
void launch_k1(const K1Args& a, const K1Plan& p, const K1WinOnce& wo, hipStream_t st, K1Log* log);
void launch_nk_simple(const int32_t* nk_raw, int32_t* nk_search, uint32_t n, int32_t min_matched, hipStream_t st);
// what the dedup stage notes about every kernel it launches (kmcpg_last_dedup_launches): written at the launch site, the template
// parameters by a launching function template of the same parameters.  nullptr = no log (and nothing else differs)
typedef std::vector<kmcpg_dedup_launch> DedupLog;
inline void dedup_note(DedupLog* log, int kernel, int p0, int p1, int p2, unsigned grid, unsigned block, int32_t lo, int32_t hi) {
  if (!log) return;
  kmcpg_dedup_launch r{};
  r.kernel = kernel;
  r.p0 = p0;
  r.p1 = p1;
  r.p2 = p2;
  r.grid = grid;
  r.block = block;
  r.lo = lo;
  r.hi = hi;
  log->push_back(r);
}
// big_bucket: KMCPG_DEDUP_BIG_BUCKET (the 16384-element distribution class); queries above HUGE_MIN are left to huge_dedup
void launch_dedup(DedupArgs a, uint64_t max_n, bool big_bucket, hipStream_t st, DedupLog* log);
// what the K2 launchers note about every kernel they launch (kmcpg_last_k2_launches): written at the launch site from the template
// parameters of the kernel launched.  nullptr = no log
typedef std::vector<kmcpg_k2_launch> K2Log;
// one launch record of the plan (k2_plan.hpp), every grid piece of it; `a` complete but for unit_base.  <0: no kernel for the record
int launch_k2(const K2Launch& l, const K2Args& a, hipStream_t st, K2Log* log);
// a pair record: two lane forms in one grid (long queries: the 64-lane tiles + the remainder's form)
int launch_k2_pair(const K2Launch& l, const K2Args& a64, const K2Args& b, hipStream_t st, K2Log* log);
// long queries: the chunked launches count into a.long_counts, then one thresholding pass
void launch_list_long(const int32_t* nk, uint32_t n_reads, int32_t split_min, uint32_t* list, uint32_t* meta, hipStream_t st);
void launch_threshold_long(const K2Args& a, hipStream_t st);
// K3: group + filter + order the hit list on the device (k3_finalize.hip); hits_hint = expected number of hits (grid sizing), 0 = hit_cap
// set != nullptr: a database set — the segments are brought into the merge order (k3_set_order.hpp) by the set forms of the sort kernels
void launch_k3(const K3Args& a, uint64_t hits_hint, hipStream_t st, const K3SetArgs* set = nullptr);
uint32_t k3_scan_tiles_for(uint32_t n);
// what K4 notes about every kernel it launches (kmcpg_last_specific); nullptr = no log
typedef std::vector<kmcpg_k4_launch> K4Log;
inline void k4_note(K4Log* log, int kernel, unsigned grid, unsigned block) {
  if (!log) return;
  kmcpg_k4_launch r{};
  r.kernel = kernel;
  r.grid = grid;
  r.block = block;
  r.cls = kernel == KMCPG_K4_VERDICT || kernel == KMCPG_K4_COMPACT || kernel == KMCPG_K5_SUMMARY || kernel == KMCPG_K5_COMPACT || kernel == KMCPG_K6_REFSTATS || kernel == KMCPG_K7_COOCCUR ||
                  kernel == KMCPG_K8_LOG || kernel == KMCPG_K8_REPLAY || kernel == KMCPG_K9_EM || kernel == KMCPG_K10_MASK || kernel == KMCPG_K10_COMPACT ||
                  kernel == KMCPG_K10_OFFS || kernel == KMCPG_K11_BIN
              ? 3
              : 0;
  log->push_back(r);
}
// the exclusive scan of K3 by itself: cnt[0 .. n) -> offs[0 .. n); sums: k3_scan_tiles_for(n) + 1 words of scratch
void launch_k3_scan(const uint32_t* cnt, uint64_t* offs, uint64_t* sums, uint32_t n, hipStream_t st, K4Log* log = nullptr);
// K4: the species-specific stage behind K3 (k4_specific.hip)
void launch_k4(const K4Args& a, hipStream_t st, K4Log* log);
// its last step alone: the segments [offs[i], offs[i] + out_offs[i + 1] - out_offs[i]) of pairs -> out_pairs at out_offs[i] (reads pairs, offs,
// n_reads, out_pairs, out_offs, out_cap)
void launch_k4_compact(const K4Args& a, hipStream_t st, K4Log* log, int kernel_id = KMCPG_K4_COMPACT);
// K5: a window's summary behind K4, the LEFT segments compacted (k5_summary.hip)
void launch_k5(const K5Args& a, hipStream_t st, K4Log* log);
// K6: the reference statistics behind K3 (k6_refstats.hip); returns the grid it launched (at most max_wgs workgroups)
unsigned launch_k6(const K6Args& a, unsigned max_wgs, hipStream_t st, K4Log* log);
// K7: the shared reads of reference pairs behind K3 (k7_cooccur.hip); returns the grid it launched (at most max_wgs workgroups)
unsigned launch_k7(const K7Args& a, unsigned max_wgs, hipStream_t st, K4Log* log);
// K8: the recount behind K3 and after the last batch (k8_recount.hip); both return the grid they launched (at most max_wgs workgroups)
unsigned launch_k8_log(const K8LogArgs& a, unsigned max_wgs, hipStream_t st, K4Log* log);
unsigned launch_k8_replay(const K8ReplayArgs& a, unsigned max_wgs, hipStream_t st, K4Log* log);
// K9: one EM pass over K8's read log (k9_em.hip); returns the grid it launched (at most max_wgs workgroups)
unsigned launch_k9_em(const K9Args& a, unsigned max_wgs, hipStream_t st, K4Log* log);
// K10: the mask of the reads the counting stages LEFT, their segments compacted (k10_left.hip)
void launch_k10(const K10Args& a, const kmcpg_pair* pairs, uint64_t* sums, uint64_t* offs_tmp, kmcpg_pair* left_pairs, uint64_t left_cap, uint64_t* left_offs,
                hipStream_t st, K4Log* log);
// K11: one TaxId per read, the LCA of its whitelisted targets (k11_bin.hip); returns the grid it launched (at most max_wgs workgroups)
unsigned launch_k11(const K11Args& a, unsigned max_wgs, hipStream_t st, K4Log* log, bool* in_lds);
void launch_max_nk(const int32_t* nk, uint32_t n_reads, unsigned long long* out, hipStream_t st);
void launch_repack(const uint8_t* src, uint8_t* dst, uint64_t n_rows, uint32_t row_bytes, uint32_t stride, uint32_t byte_off, uint32_t ncols, hipStream_t st);
void launch_gather_rows(const uint8_t* rows, uint32_t stride, uint32_t row_bytes, const uint64_t* idx, uint64_t first, uint64_t n, uint8_t* out,
                        hipStream_t st);
void launch_synth_fill(uint8_t* rows, uint64_t n_rows, uint32_t stride, uint32_t own_stride, uint32_t ncols, uint64_t key, uint32_t p8, hipStream_t st);
void launch_plant(const BlockDev& bd, uint32_t col, int num_hashes, const uint64_t* hashes, uint64_t n, hipStream_t st);

void launch_plant_reads(const BlockDev* blocks, uint32_t nblocks, int num_hashes, const uint64_t* hashes, const uint64_t* offs,
                        const int32_t* nk, const uint32_t* cols, uint32_t n_reads, hipStream_t st);

void launch_build_scatter(uint8_t* sigs, uint64_t num_sigs, uint64_t mh, uint32_t row_bytes, int num_hashes, const uint64_t* hashes,
                          const uint64_t* col_off, uint32_t col0, uint32_t n_cols, uint64_t n, hipStream_t st);

// 2-bit packed bases (4 per byte, base j in bits 2*(j%4) of byte j/4; A=0 C=1 T=2 G=3 = (ascii >> 1) & 3) -> ASCII, then the
// exception runs (every byte that is not A/C/G/T/U in either case) written over them
void launch_unpack2(const uint8_t* packed, uint8_t* out, uint64_t n_bases, const ExcRun* runs, uint32_t n_runs, hipStream_t st);
void launch_apply_exc(const ExcRun* runs, uint32_t n_runs, uint8_t* out, hipStream_t st);  // the runs alone, over text that is there

// sliding windows (windows.hip): descriptors of n_win windows over n_slices staged slices of reads (soffs: the slices' bases in the staged
// text, wpre / vpre: prefix sums of their windows and of those windows' bases) -> src[w] (first base in the text), offs[0 .. n_win]
void launch_window_desc(const uint64_t* soffs, const uint64_t* wpre, const uint64_t* vpre, uint32_t n_slices, uint64_t n_win, uint64_t step,
                        uint64_t window, uint64_t* src, uint64_t* offs, hipStream_t st);

// index inspection (density.hip): set bits per (column, row bin) of 16-byte lanes lane0 .. lane0 + nlanes - 1 of resident rows,
// rows first_row .. last_row - 1, bins of bin_rows rows from first_row.  out[bin * width + 128 * (lane - lane0) + column of the lane],
// zero on entry (bins shared by several waves are added to).  plan_density (density_core.hpp) decides the form and the grid; the host sizes `out` from it.
int launch_density(const DensityPlan& p, DensityArgs a, hipStream_t st);  // <0 on bad arguments
// in[b * width + col0 + c] -> out[c * nb + b] for c < ncols, b < nb
void launch_density_transpose(const uint32_t* in, uint64_t width, uint32_t col0, uint32_t ncols, uint64_t nb, uint32_t* out, hipStream_t st);
// one bin over a whole group's row (lane0 = 0) -> ones[global column] of the group's members
void launch_density_cols(const uint32_t* in, const Seg* segs, uint32_t nsegs, uint32_t max_ncols, uint64_t* ones, hipStream_t st);

// bench support: `bytes` of device memory read once, 16 B per lane, one XOR per load (out: one word, never written in practice)
void launch_stream_probe(const uint8_t* buf, uint64_t bytes, uint32_t* out, hipStream_t st);

// experiment only (KMCPG_DEBUG_ROWSORT): every query's hashes re-ordered by h % num_sigs of one block; mode 2 = rotated
void launch_debug_rowsort(uint64_t* hashes, const uint64_t* offs, const int32_t* nk, uint32_t n_reads, uint64_t num_sigs, uint64_t mh, int mode, hipStream_t st);

// queries of up to this many emissions above -u are sorted by one wave (k_dedup_wave), which reads them from hashes[]; the
// long-read sketch kernels keep the raw emissions of such queries for it (k1_reads.hip, k1_windows.hip)
constexpr int DEDUP_WAVE_CAP = 512;
// queries with more than HUGE_MIN k-mers: device-wide sort + unique (sort_huge.hip)
constexpr uint32_t HUGE_MIN = 65536;
size_t huge_dedup_temp_bytes(uint32_t max_n);
void launch_gather_huge(const uint32_t* list, uint32_t n, const int32_t* nk_raw, const uint64_t* offs, const uint64_t* offs2, uint64_t* out,
                        hipStream_t st);
int huge_dedup(uint64_t* keys, uint64_t* tmp, uint32_t n, int* d_num, void* d_temp, size_t temp_bytes, int32_t* nk_search, uint32_t r, int min_matched,
               hipStream_t st, DedupLog* log);

}  // namespace kmcpg
