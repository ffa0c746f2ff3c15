"""ctypes binding of libkmcpgpu.so (include/kmcp_gpu.h).

Plumbing only: the product is the shared library.  There is no CPU fallback — if the library is missing
or no GPU is present, every compute entry point raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkmcpgpu.so")

EXPORTS = [
    "kmcpg_open", "kmcpg_close", "kmcpg_last_error", "kmcpg_db_info", "kmcpg_col_info", "kmcpg_search_batch",
    "kmcpg_result_free", "kmcpg_query_device", "kmcpg_finalize", "kmcpg_open_synthetic", "kmcpg_plant",
    "kmcpg_read_rows", "kmcpg_block_info", "kmcpg_kmers_device", "kmcpg_plant_reads_device", "kmcpg_set_profiling",
    "kmcpg_last_timing", "kmcpg_open_devices", "kmcpg_build_db", "kmcpg_submit", "kmcpg_wait", "kmcpg_read_row_range", "kmcpg_timing_at", "kmcpg_last_gathered_bytes", "kmcpg_last_hash_bytes", "kmcpg_last_tail_waves", "kmcpg_last_k2_launches",
    "kmcpg_db_ks", "kmcpg_open_paged", "kmcpg_paged_info", "kmcpg_exchange_info", "kmcpg_batch_hint", "kmcpg_group_device", "kmcpg_finalize_grouped",
    "kmcpg_search_batch_pairs", "kmcpg_wait_pairs", "kmcpg_result_pairs_free", "kmcpg_expand_pairs", "kmcpg_save_db",
    "kmcpg_pack2", "kmcpg_unpack2", "kmcpg_submit_packed", "kmcpg_host_alloc", "kmcpg_host_free",
    "kmcpg_kmers_device_packed", "kmcpg_k1_codes_batches", "kmcpg_kmers_device_paired", "kmcpg_last_k1_launches",
    "kmcpg_submit_windows", "kmcpg_submit_packed_windows", "kmcpg_window_count", "kmcpg_window_locate", "kmcpg_kmers_device_windows",
    "kmcpg_density_bins", "kmcpg_block_density", "kmcpg_col_ones", "kmcpg_last_density_launch", "kmcpg_open_files",
    "kmcpg_last_density_ms", "kmcpg_stream_probe",
    "kmcpg_sketcher_open", "kmcpg_sketcher_close", "kmcpg_split_bounds", "kmcpg_sketch_genomes", "kmcpg_sketch_result_free",
    "kmcpg_last_sketch_launches", "kmcpg_last_sketch_ms", "kmcpg_sort_segments_device", "kmcpg_dedup_device", "kmcpg_last_dedup_launches",
    "kmcpg_open_set", "kmcpg_set_info", "kmcpg_last_set_order",
    "kmcpg_set_specific", "kmcpg_specific_device", "kmcpg_last_specific",
    "kmcpg_summarize_device", "kmcpg_last_summary", "kmcpg_submit_windows_summary", "kmcpg_wait_summaries", "kmcpg_result_summaries_free",
    "kmcpg_set_refstats", "kmcpg_refstats_device", "kmcpg_refstats_read", "kmcpg_refstats_reset", "kmcpg_last_refstats",
    "kmcpg_set_cooccur", "kmcpg_cooccur_device", "kmcpg_cooccur_read", "kmcpg_cooccur_reset", "kmcpg_last_cooccur",
    "kmcpg_set_recount", "kmcpg_recount_log_device", "kmcpg_recount_run", "kmcpg_recount_read", "kmcpg_recount_reset", "kmcpg_last_recount",
    "kmcpg_em_pass", "kmcpg_em_read", "kmcpg_last_em", "kmcpg_count_left_reads",
    "kmcpg_left_compact_device", "kmcpg_submit_stats", "kmcpg_wait_stats", "kmcpg_last_stats",
    "kmcpg_set_binning", "kmcpg_bin_device", "kmcpg_last_bins", "kmcpg_submit_bins", "kmcpg_wait_bins",
    "kmcpg_sketch_genomes_to", "kmcpg_builder_open", "kmcpg_builder_close", "kmcpg_builder_add_cols", "kmcpg_builder_plan",
    "kmcpg_builder_col_place", "kmcpg_builder_block_info", "kmcpg_builder_begin_round", "kmcpg_builder_scatter_device",
    "kmcpg_builder_end_round", "kmcpg_builder_finish", "kmcpg_builder_info",
]


def pack2(pieces, codes=None, exc=None, pos=0):
    """kmcpg_pack2 over a list of byte strings / uint8 arrays appended one after the other from base position `pos`:
    returns (codes uint8[(total + 3) // 4 + 8], exc EXC_DTYPE[n_exc], total bases)."""
    arrs = [np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8) for x in pieces]
    total = pos + sum(len(a) for a in arrs)
    if codes is None:
        codes = np.zeros((total + 3) // 4 + 8, dtype=np.uint8)
    cap = 1024 if exc is None else max(1024, 2 * len(exc))
    runs = np.zeros(cap, dtype=EXC_DTYPE)
    n_exc = C.c_uint64(0)
    if exc is not None and len(exc):
        runs[:len(exc)] = exc
        n_exc.value = len(exc)
    at = pos
    for a in arrs:
        while True:
            before = n_exc.value
            rc = load().kmcpg_pack2(a.ctypes.data, len(a), at, codes.ctypes.data, runs.ctypes.data, len(runs), C.byref(n_exc))
            if rc == 0:
                break
            if rc != -5:
                _check(rc)
            grown = np.zeros(max(2 * len(runs), int(n_exc.value) + 1024), dtype=EXC_DTYPE)
            grown[:before] = runs[:before]
            runs = grown
            n_exc.value = before
        at += len(a)
    return codes, runs[:n_exc.value].copy(), total


class PinnedBytes:
    """uint8 array in page-locked memory from kmcpg_host_alloc (`.a`); freed by close() / the context manager."""

    def __init__(self, n):
        self._p = C.c_void_p()
        _check(load().kmcpg_host_alloc(n, C.byref(self._p)))
        self.a = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_uint8)), shape=(max(int(n), 64),))

    def close(self):
        if self._p:
            self.a = None
            _check(load().kmcpg_host_free(self._p))
            self._p = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def unpack2(codes, n_bases, exc):
    out = np.empty(n_bases, dtype=np.uint8)
    _check(load().kmcpg_unpack2(codes.ctypes.data, n_bases, exc.ctypes.data if len(exc) else None, len(exc), out.ctypes.data))
    return out


class KmcpGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libkmcpgpu error {code}: {msg}")
        self.code = code


class Opts(C.Structure):
    _fields_ = [("device", C.c_int32), ("shard_rank", C.c_int32), ("shard_count", C.c_int32), ("reserved", C.c_int32)]


class Info(C.Structure):
    _fields_ = [("k", C.c_int32), ("canonical", C.c_int32), ("num_hashes", C.c_int32), ("scaled", C.c_int32),
                ("scale", C.c_uint32), ("minimizer", C.c_int32), ("minimizer_w", C.c_uint32), ("syncmer", C.c_int32),
                ("syncmer_s", C.c_uint32), ("fpr", C.c_double), ("n_blocks", C.c_int32), ("n_blocks_local", C.c_int32),
                ("n_cols", C.c_uint64), ("matrix_bytes", C.c_uint64), ("matrix_bytes_local", C.c_uint64),
                ("row_bytes_sum_local", C.c_uint64)]


class Params(C.Structure):
    _fields_ = [("min_qlen", C.c_int32), ("min_matched", C.c_int32), ("min_qcov", C.c_double), ("min_tcov", C.c_double),
                ("max_fpr", C.c_double), ("dedup_threshold", C.c_int32), ("try_se", C.c_int32), ("sort_by", C.c_int32),
                ("do_not_sort", C.c_int32), ("top_n_scores", C.c_int32), ("fpr_buf_size", C.c_int32), ("k", C.c_int32),
                ("reserved", C.c_int32)]


class Hit(C.Structure):
    _fields_ = [("read", C.c_uint32), ("col", C.c_uint32), ("count", C.c_uint32)]


class Match(C.Structure):
    _fields_ = [("col", C.c_uint32), ("target_idx", C.c_uint32), ("gsize", C.c_uint64), ("mkmers", C.c_int32),
                ("reserved", C.c_int32), ("fpr", C.c_double), ("qcov", C.c_double), ("tcov", C.c_double), ("jacc", C.c_double)]


class Result(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("k", C.c_int32), ("qlen", C.POINTER(C.c_int32)), ("qkmers", C.POINTER(C.c_int32)),
                ("ksize", C.POINTER(C.c_int32)), ("match_offs", C.POINTER(C.c_uint64)), ("matches", C.POINTER(Match)), ("owner", C.c_void_p)]


class WindowSpec(C.Structure):
    """kmcpg_window_spec: seqkit sliding -s step -W window [-g]"""
    _fields_ = [("step", C.c_uint64), ("window", C.c_uint64), ("greedy", C.c_int32), ("reserved", C.c_int32)]


class K2Launch(C.Structure):
    """kmcpg_k2_launch: one COBS kernel launch of a query_device call"""
    _fields_ = [("kind", C.c_int32), ("lpr", C.c_int32), ("lprb", C.c_int32), ("npl", C.c_int32), ("multi", C.c_int32),
                ("group_rows", C.c_int32), ("workgroups", C.c_uint32), ("grid", C.c_uint32)]


K2_KINDS = ("plain", "split", "pair")


class K1Launch(C.Structure):
    """kmcpg_k1_launch: one K1 kernel launch of a k-mer stage, or (kernel 0) the plan of that stage"""
    _fields_ = [("kernel", C.c_int32), ("p0", C.c_int32), ("p1", C.c_int32), ("grid", C.c_uint32), ("block", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("left_on_list", C.c_uint32), ("reserved", C.c_uint32)]


# KMCPG_K1_* and KMCPG_K1F_* (include/kmcp_gpu.h)
K1_KERNELS = ("plan", "k1_kmers", "k1_kmers_wg", "k1_kmers_wg_global", "k1_windows_wave", "k1_windows_roll", "k1_seg_roll2", "k1_seg_roll",
              "k1_seg_hash", "k1_seg_pack", "k_mark_exc", "k_unpack2_list", "k1_win_hash", "k1_win_scan", "k1_win_rank", "k1_win_gather")
K1_FORMS = ("None", "WinOnce", "SegRoll2", "SegRoll", "SegHash", "WindowsRoll", "WindowsWave", "WgGlobal", "Wg", "Short")


class DedupSpec(C.Structure):
    """kmcpg_dedup_spec: the five scalars of the dedup stage (-u, -m, and DedupArgs' pre / pre_done / key_shift)"""
    _fields_ = [("dedup_threshold", C.c_int32), ("min_matched", C.c_int32), ("pre", C.c_int32), ("pre_done", C.c_int32), ("key_shift", C.c_int32)]


class DedupLaunch(C.Structure):
    """kmcpg_dedup_launch: one kernel launch of a dedup stage, or (first record) the branch the stage took"""
    _fields_ = [("kernel", C.c_int32), ("p0", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("grid", C.c_uint32), ("block", C.c_uint32),
                ("lo", C.c_int32), ("hi", C.c_int32)]


# KMCPG_DD_* (include/kmcp_gpu.h)
DEDUP_KERNELS = ("launch_dedup", "k_nk_simple", "k_dedup_wave", "k_adj_unique", "k_dedup_bucket", "k_dedup", "k_rs_hist", "k_scan_tile_sums",
                 "k_scan_u32", "k_scan_tiles", "k_rs_scatter", "k_uq_count", "k_uq_scatter", "k_set_nk_huge")


class DensitySpec(C.Structure):
    """kmcpg_density_spec: rows first_row .. (n_rows of them, 0 = to the end) in bins of bin_rows rows"""
    _fields_ = [("bin_rows", C.c_uint64), ("first_row", C.c_uint64), ("n_rows", C.c_uint64), ("reserved", C.c_uint64)]


class DensityLaunch(C.Structure):
    """kmcpg_density_launch: what the last density call launched"""
    _fields_ = [("form", C.c_int32), ("lpr", C.c_int32), ("npl", C.c_int32), ("reserved", C.c_int32), ("workgroups", C.c_uint32),
                ("launches", C.c_uint32)]


DENSITY_FORMS = ("csa", "small")


class SketchCfg(C.Structure):
    """kmcpg_sketch_cfg: the sketch of `kmcp compute` (always canonical)"""
    _fields_ = [("ks", C.c_int32 * 8), ("n_k", C.c_int32), ("scale", C.c_uint32), ("minimizer_w", C.c_uint32), ("syncmer_s", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class SplitSpec(C.Structure):
    """kmcpg_split_spec: -n / -l / -m of `kmcp compute`, and the smallest / largest k of the sketch"""
    _fields_ = [("split_number", C.c_uint32), ("split_overlap", C.c_uint32), ("split_min_ref", C.c_uint64), ("k_min", C.c_int32),
                ("k_max", C.c_int32), ("reserved", C.c_uint64)]


class SketchResult(C.Structure):
    _fields_ = [("n_chunks", C.c_uint32), ("reserved", C.c_uint32), ("genome", C.POINTER(C.c_uint32)), ("chunk_idx", C.POINTER(C.c_uint32)),
                ("chunks", C.POINTER(C.c_uint32)), ("koff", C.POINTER(C.c_uint64)), ("hashes", C.POINTER(C.c_uint64)), ("owner", C.c_void_p)]


class SketchLaunch(C.Structure):
    """kmcpg_sketch_launch: the segmented sort of one piece of a sketch_genomes call"""
    _fields_ = [("kind", C.c_int32), ("passes", C.c_int32), ("key_bits", C.c_int32), ("segments", C.c_uint32), ("workgroups", C.c_uint32),
                ("launches", C.c_uint32), ("keys", C.c_uint64)]


class SetOrder(C.Structure):
    """kmcpg_set_order: what put the segments of a set handle's last batch into the merge order"""
    _fields_ = [("wave_segments", C.c_uint64), ("wg_segments", C.c_uint64), ("long_segments", C.c_uint64), ("device_mixed_runs", C.c_uint64),
                ("host_segments", C.c_uint64), ("host_mixed_runs", C.c_uint64)]


class K4Launch(C.Structure):
    """kmcpg_k4_launch: one kernel launch of the species-specific stage"""
    _fields_ = [("kernel", C.c_int32), ("grid", C.c_uint32), ("block", C.c_uint32), ("cls", C.c_int32)]


# KMCPG_K4_* and KMCPG_SPECIFIC_* (include/kmcp_gpu.h)
K4_VERDICT, K4_SCAN_TILES, K4_SCAN_SUMS, K4_SCAN_ADD, K4_COMPACT = range(5)
SPECIFIC_DROP, SPECIFIC_KEEP, SPECIFIC_HOST = 0, 1, 2


class SpecificStats(C.Structure):
    """kmcpg_specific_stats: the witness of the last K4 launch"""
    _fields_ = [("kept", C.c_uint64), ("dropped", C.c_uint64), ("host", C.c_uint64), ("pairs_in", C.c_uint64), ("pairs_out", C.c_uint64),
                ("group_segments", C.c_uint64), ("wave_segments", C.c_uint64), ("bad_segments", C.c_uint64), ("k4_ms", C.c_double)]


class WindowSummary(C.Structure):
    """kmcpg_window_summary: what region merging needs of one window"""
    _fields_ = [("n_targets", C.c_uint32), ("flags", C.c_uint32), ("score", C.c_double)]


SUMMARY_DTYPE = np.dtype([("n_targets", "<u4"), ("flags", "<u4"), ("score", "<f8")])
SUMMARY_LEFT, SUMMARY_HOST = 1, 2
K5_SUMMARY, K5_COMPACT = 16, 17  # KMCPG_K5_*: kmcpg_k4_launch.kernel of K5's own kernels


class SummaryStats(C.Structure):
    """kmcpg_summary_stats: the witness of the last K5 launch, or of the last ticket of wait_summaries"""
    _fields_ = [("single", C.c_uint64), ("wave", C.c_uint64), ("left", C.c_uint64), ("empty", C.c_uint64), ("left_pairs", C.c_uint64),
                ("bytes_d2h", C.c_uint64), ("bad_segments", C.c_uint64), ("k5_ms", C.c_double)]


K10_MASK, K10_COMPACT, K10_OFFS = 67, 68, 69  # KMCPG_K10_*: kmcpg_k4_launch.kernel of K10's own kernels


class StatsResult(C.Structure):
    """kmcpg_result_stats: what a statistics-only ticket came to (plain values, nothing to free)"""
    _fields_ = [("n_reads", C.c_uint64), ("matched_reads", C.c_uint64), ("kept_pairs", C.c_uint64), ("left_reads", C.c_uint64),
                ("left_pairs", C.c_uint64), ("bytes_d2h", C.c_uint64)]


class StatsTicketStats(C.Structure):
    """kmcpg_stats_ticket_stats: the witness of the last K10 launch, or of the last ticket of wait_stats"""
    _fields_ = [("n_reads", C.c_uint64), ("matched_reads", C.c_uint64), ("kept_pairs", C.c_uint64), ("left_reads", C.c_uint64),
                ("left_pairs", C.c_uint64), ("bytes_d2h", C.c_uint64), ("bad_segments", C.c_uint64), ("skipped", C.c_uint64), ("k10_ms", C.c_double)]


K11_BIN = 70  # KMCPG_K11_BIN: kmcpg_k4_launch.kernel of K11's kernel
BIN_NO_NODE, BIN_NONE, BIN_LEFT = 0xffffffff, 0xffffffff, 0xfffffffe  # KMCPG_BIN_*


class BinsResult(C.Structure):
    """kmcpg_result_bins: what a binning ticket came to (plain values, nothing to free)"""
    _fields_ = [("n_reads", C.c_uint64), ("binned_reads", C.c_uint64), ("kept_pairs", C.c_uint64), ("host_reads", C.c_uint64),
                ("left_pairs", C.c_uint64), ("bytes_d2h", C.c_uint64), ("reruns", C.c_uint64)]


class BinTicket(C.c_void_p):
    """a ticket of submit_bins: the handle's pointer, and the reads it stands for (wait_bins sizes its output by it)"""
    n_reads = 0


class BinStats(C.Structure):
    """kmcpg_bin_stats: the witness of the last K11 launch"""
    _fields_ = [("no_bin", C.c_uint64), ("one", C.c_uint64), ("several", C.c_uint64), ("left", C.c_uint64), ("climb_steps", C.c_uint64),
                ("bad_segments", C.c_uint64), ("skipped", C.c_uint64), ("grid", C.c_uint32), ("in_lds", C.c_uint32), ("k11_ms", C.c_double)]


COL_STATS_DTYPE = np.dtype([("rows", "<u8"), ("firsts", "<u8"), ("ureads", "<u8"), ("hic_ureads", "<u8")])  # kmcpg_col_stats
K6_REFSTATS = 32  # KMCPG_K6_REFSTATS: kmcpg_k4_launch.kernel of K6's kernel


class RefstatsTotals(C.Structure):
    """kmcpg_refstats_totals"""
    _fields_ = [("matched_reads", C.c_uint64), ("unique_reads", C.c_uint64), ("host_reads", C.c_uint64), ("skipped_launches", C.c_uint64)]


class RefstatsStats(C.Structure):
    """kmcpg_refstats_stats: the witness of the last K6 launch"""
    _fields_ = [("empty", C.c_uint64), ("single", C.c_uint64), ("wave", C.c_uint64), ("left", C.c_uint64), ("lds_adds", C.c_uint64),
                ("global_adds", C.c_uint64), ("spilled_adds", C.c_uint64), ("skipped", C.c_uint64), ("bad_segments", C.c_uint64),
                ("grid", C.c_uint32), ("slots", C.c_uint32), ("k6_ms", C.c_double)]


COOCCUR_DTYPE = np.dtype([("class_a", "<u4"), ("class_b", "<u4"), ("reads", "<u8")])  # kmcpg_cooccur_pair
K7_COOCCUR = 48  # KMCPG_K7_COOCCUR: kmcpg_k4_launch.kernel of K7's kernel


class CooccurTotals(C.Structure):
    """kmcpg_cooccur_totals"""
    _fields_ = [("multi_reads", C.c_uint64), ("device_adds", C.c_uint64), ("host_adds", C.c_uint64), ("left_full", C.c_uint64),
                ("host_reads", C.c_uint64), ("skipped_launches", C.c_uint64), ("table_slots", C.c_uint64), ("keys", C.c_uint64),
                ("rebuilds", C.c_uint64)]


class CooccurStats(C.Structure):
    """kmcpg_cooccur_stats: the witness of the last K7 launch"""
    _fields_ = [("empty", C.c_uint64), ("single", C.c_uint64), ("wave", C.c_uint64), ("left", C.c_uint64), ("left_full", C.c_uint64),
                ("pairs", C.c_uint64), ("lds_adds", C.c_uint64), ("global_adds", C.c_uint64), ("spilled_adds", C.c_uint64),
                ("claimed", C.c_uint64), ("skipped", C.c_uint64), ("bad_segments", C.c_uint64), ("grid", C.c_uint32), ("slots", C.c_uint32),
                ("k7_ms", C.c_double)]


RECOUNT_DTYPE = np.dtype([("match", "<u8"), ("uniq", "<u8"), ("hic", "<u8"), ("bases", "<u8")])  # kmcpg_recount_col, in units
RECOUNT_CLASS_DTYPE = np.dtype([("kept", "<u4"), ("reserved", "<u4"), ("reads", "<u8"), ("ureads", "<u8")])  # kmcpg_recount_class
RECOUNT_UNIT, RECOUNT_BASE_UNIT = 720720, 65536  # recount_rule.hpp: units per read, per base
K8_LOG, K8_REPLAY = 64, 65  # KMCPG_K8_LOG, KMCPG_K8_REPLAY: kmcpg_k4_launch.kernel of K8's kernels


class RecountParams(C.Structure):
    """kmcpg_recount_params"""
    _fields_ = [("one_minus_d", C.c_double), ("r_err", C.c_double), ("no_amb_corr", C.c_uint32), ("level_species", C.c_uint32)]


class RecountTotals(C.Structure):
    """kmcpg_recount_totals"""
    _fields_ = [("recounted_reads", C.c_uint64), ("unique_reads", C.c_uint64), ("corrected_reads", C.c_uint64), ("single_reads", C.c_uint64),
                ("replayed_reads", C.c_uint64), ("host_reads", C.c_uint64), ("left_full", C.c_uint64), ("skipped_launches", C.c_uint64),
                ("log_bytes", C.c_uint64), ("log_bytes_used", C.c_uint64), ("logged_reads", C.c_uint64)]


class RecountStats(C.Structure):
    """kmcpg_recount_stats: the witness of the last k8_log launch and of the last replay"""
    _fields_ = [("empty", C.c_uint64), ("single", C.c_uint64), ("logged", C.c_uint64), ("left", C.c_uint64), ("left_full", C.c_uint64),
                ("lds_adds", C.c_uint64), ("global_adds", C.c_uint64), ("spilled_adds", C.c_uint64), ("skipped", C.c_uint64),
                ("bad_segments", C.c_uint64), ("log_bytes_used", C.c_uint64), ("replay_reads", C.c_uint64), ("replay_recounted", C.c_uint64),
                ("replay_corrected", C.c_uint64), ("replay_unique", C.c_uint64), ("replay_lookups", C.c_uint64), ("replay_lds_adds", C.c_uint64),
                ("replay_global_adds", C.c_uint64), ("replay_spilled_adds", C.c_uint64), ("grid", C.c_uint32), ("slots", C.c_uint32),
                ("replay_grid", C.c_uint32), ("reserved", C.c_uint32), ("log_ms", C.c_double), ("replay_ms", C.c_double)]


EM_COL_DTYPE = np.dtype([("match", "<u8"), ("uniq", "<u8"), ("hic", "<u8"), ("single_bases", "<u8"), ("bases_lo", "<u8"), ("bases_hi", "<u8")])  # kmcpg_em_col
EM_CLASS_DTYPE = np.dtype([("est", "<u4"), ("reserved", "<u4"), ("coverage", "<f8")])  # kmcpg_em_class
EM_UNIT = RECOUNT_UNIT << 12  # em_rule.hpp: units per read of an EM pass
K9_EM = 66  # KMCPG_K9_EM: kmcpg_k4_launch.kernel of K9


class EmTotals(C.Structure):
    """kmcpg_em_totals"""
    _fields_ = [("assigned_reads", C.c_uint64), ("unique_reads", C.c_uint64), ("split_reads", C.c_uint64), ("host_reads", C.c_uint64)]


class EmStats(C.Structure):
    """kmcpg_em_stats: the witness of the last k9_em launch"""
    _fields_ = [("reads", C.c_uint64), ("none", C.c_uint64), ("one", C.c_uint64), ("split", C.c_uint64), ("lds_adds", C.c_uint64),
                ("global_adds", C.c_uint64), ("spilled_adds", C.c_uint64), ("grid", C.c_uint32), ("slots", C.c_uint32), ("em_ms", C.c_double)]


class ResultSummaries(C.Structure):
    """kmcpg_result_summaries"""
    _fields_ = [("n_windows", C.c_uint32), ("reserved", C.c_uint32), ("qlen", C.POINTER(C.c_int32)), ("qkmers", C.POINTER(C.c_int32)),
                ("s", C.POINTER(WindowSummary)), ("owner", C.c_void_p)]


class SynthSpec(C.Structure):
    _fields_ = [("k", C.c_int32), ("num_hashes", C.c_int32), ("fpr", C.c_double), ("n_blocks", C.c_uint32),
                ("cols_per_block", C.c_uint32), ("num_sigs", C.c_uint64), ("kmers_per_col", C.c_uint64), ("seed", C.c_uint64),
                ("scale", C.c_uint32), ("syncmer_s", C.c_uint32), ("minimizer_w", C.c_uint32), ("sigs_step", C.c_uint32)]


class BuildCfg(C.Structure):
    _fields_ = [("k", C.c_int32), ("canonical", C.c_int32), ("num_hashes", C.c_int32), ("fpr", C.c_double), ("threads", C.c_int32),
                ("block_size", C.c_int32), ("scale", C.c_uint32), ("minimizer_w", C.c_uint32), ("syncmer_s", C.c_uint32),
                ("split_seq", C.c_int32), ("split_size", C.c_int32), ("split_num", C.c_int32), ("split_overlap", C.c_int32),
                ("alias", C.c_char_p), ("kmers_x", C.c_uint64), ("block_size_x", C.c_int32), ("uniform_sigs", C.c_int32), ("kmers_8", C.c_uint64),
                ("kmers_1", C.c_uint64)]


class BuildCol(C.Structure):
    _fields_ = [("name", C.c_char_p), ("gsize", C.c_uint64), ("chunk_idx", C.c_uint32), ("chunks", C.c_uint32),
                ("hashes", C.c_void_p), ("n_hashes", C.c_uint64)]


class BuilderCfg(C.Structure):
    _fields_ = [("build", BuildCfg), ("hbm_reserve", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class BuildColMeta(C.Structure):
    _fields_ = [("name", C.c_char_p), ("gsize", C.c_uint64), ("chunk_idx", C.c_uint32), ("chunks", C.c_uint32), ("n_hashes", C.c_uint64)]


class BuilderStats(C.Structure):
    _fields_ = [("rounds_done", C.c_uint32), ("slice_keys", C.c_uint32), ("scatter_calls", C.c_uint64), ("scatter_launches", C.c_uint64),
                ("keys_scattered", C.c_uint64), ("lists_skipped", C.c_uint64), ("matrix_bytes_resident", C.c_uint64),
                ("matrix_bytes_peak", C.c_uint64), ("scatter_ms", C.c_double), ("reserved", C.c_uint64 * 2)]


class SketchPiece(C.Structure):
    _fields_ = [("first_chunk", C.c_uint32), ("n_chunks", C.c_uint32), ("genome", C.POINTER(C.c_uint32)), ("chunk_idx", C.POINTER(C.c_uint32)),
                ("chunks", C.POINTER(C.c_uint32)), ("koff", C.POINTER(C.c_uint64)), ("d_hashes", C.c_void_p), ("stream", C.c_void_p)]


SKETCH_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(SketchPiece))

HIT_DTYPE = np.dtype([("read", np.uint32), ("col", np.uint32), ("count", np.uint32)])
PAIR_DTYPE = np.dtype([("col", np.uint32), ("count", np.uint32)])
EXC_DTYPE = np.dtype([("pos", np.uint64), ("len", np.uint32), ("byte", np.uint32)])  # kmcpg_exc_run
MATCH_DTYPE = np.dtype([("col", np.uint32), ("target_idx", np.uint32), ("gsize", np.uint64), ("mkmers", np.int32),
                        ("reserved", np.int32), ("fpr", np.float64), ("qcov", np.float64), ("tcov", np.float64),
                        ("jacc", np.float64)])
assert HIT_DTYPE.itemsize == C.sizeof(Hit) and MATCH_DTYPE.itemsize == C.sizeof(Match)


def default_params(**kw):
    """Defaults of `kmcp search` (kmcp/cmd/search.go:1052-1102)."""
    p = Params(min_qlen=30, min_matched=10, min_qcov=0.55, min_tcov=0.0, max_fpr=0.01, dedup_threshold=256, try_se=0,
               sort_by=0, do_not_sort=0, top_n_scores=0, fpr_buf_size=0, k=0, reserved=0)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


_lib = None


def load():
    """Load libkmcpgpu.so; raises if it has not been built (there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). kmcp_amd has no CPU fallback.")
    # PyTorch-ROCm bundles its own HIP/HSA runtime under the soname libamdhip64.so.7.  Two HIP runtimes in
    # one process cannot both own the GPU, so torch's copy must be mapped first; libkmcpgpu.so's NEEDED entry
    # then binds to it.  (Stand-alone C/C++/Go hosts simply get /opt/rocm's runtime.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u64p, i32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    L.kmcpg_last_error.restype = C.c_char_p
    L.kmcpg_open.argtypes = [C.c_char_p, C.POINTER(Opts), C.POINTER(vp)]
    L.kmcpg_open_synthetic.argtypes = [C.POINTER(SynthSpec), C.POINTER(Opts), C.POINTER(vp)]
    L.kmcpg_open_devices.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(vp)]
    L.kmcpg_open_paged.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.kmcpg_paged_info.argtypes = [vp, i32p, u64p]
    L.kmcpg_exchange_info.argtypes = [vp]
    L.kmcpg_batch_hint.argtypes = [vp, u64p]
    L.kmcpg_exchange_info.restype = C.c_char_p
    L.kmcpg_close.argtypes = [vp]
    L.kmcpg_db_info.argtypes = [vp, C.POINTER(Info)]
    L.kmcpg_db_ks.argtypes = [vp, i32p, C.c_int32, i32p]
    L.kmcpg_col_info.argtypes = [vp, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), u64p, u64p]
    L.kmcpg_block_info.argtypes = [vp, C.c_uint32, u64p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint32), i32p, C.POINTER(C.c_uint32)]
    L.kmcpg_search_batch.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.POINTER(Params), C.POINTER(Result)]
    L.kmcpg_result_free.argtypes = [C.POINTER(Result)]
    L.kmcpg_result_free.restype = None
    L.kmcpg_submit.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.POINTER(Params), C.POINTER(vp)]
    L.kmcpg_wait.argtypes = [vp, C.POINTER(Result)]
    L.kmcpg_query_device.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(Params), vp,
                                     C.c_uint64, vp, vp, vp, vp]
    L.kmcpg_finalize.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.POINTER(Params), C.POINTER(Result)]
    L.kmcpg_group_device.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.POINTER(Params), vp, vp, vp]
    L.kmcpg_finalize_grouped.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.POINTER(Params), C.POINTER(Result)]
    L.kmcpg_search_batch_pairs.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.POINTER(Params), C.POINTER(ResultPairs)]
    L.kmcpg_wait_pairs.argtypes = [vp, C.POINTER(ResultPairs)]
    L.kmcpg_result_pairs_free.argtypes = [C.POINTER(ResultPairs)]
    L.kmcpg_result_pairs_free.restype = None
    L.kmcpg_expand_pairs.argtypes = [vp, C.c_int32, vp, C.c_uint64, vp]
    L.kmcpg_plant.argtypes = [vp, C.c_uint32, vp, C.c_uint64]
    L.kmcpg_read_rows.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp]
    L.kmcpg_read_row_range.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, vp]
    L.kmcpg_kmers_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(Params), vp, C.c_uint64,
                                     vp, vp, vp]
    L.kmcpg_kmers_device_packed.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(Params), vp, C.c_uint64,
                                            vp, vp, vp]
    L.kmcpg_k1_codes_batches.argtypes = [vp, u64p, u64p]
    L.kmcpg_plant_reads_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, vp, vp]
    L.kmcpg_set_profiling.argtypes = [vp, C.c_int]
    L.kmcpg_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.kmcpg_last_gathered_bytes.argtypes = [vp, u64p]
    L.kmcpg_last_tail_waves.argtypes = [vp, u64p]
    L.kmcpg_last_hash_bytes.argtypes = [vp, u64p]
    L.kmcpg_last_k2_launches.argtypes = [vp, C.POINTER(K2Launch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_last_k1_launches.argtypes = [vp, C.POINTER(K1Launch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_kmers_device_paired.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(Params), vp, C.c_uint64, vp, vp, vp]
    L.kmcpg_kmers_device_windows.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32,
                                             C.POINTER(WindowSpec), C.POINTER(Params), vp, C.c_uint64, vp, vp, vp, vp, vp]
    L.kmcpg_timing_at.argtypes =[vp, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.kmcpg_build_db.argtypes = [C.c_char_p, C.POINTER(BuildCfg), C.POINTER(BuildCol), C.c_uint32, C.c_int32]
    L.kmcpg_save_db.argtypes = [vp, C.c_char_p]
    L.kmcpg_pack2.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, u64p]
    L.kmcpg_unpack2.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp]
    L.kmcpg_host_alloc.argtypes = [C.c_uint64, C.POINTER(vp)]
    L.kmcpg_host_free.argtypes = [vp]
    L.kmcpg_submit_packed.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint32, C.POINTER(Params), C.POINTER(vp)]
    L.kmcpg_submit_windows.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(WindowSpec), C.POINTER(Params), C.POINTER(vp)]
    L.kmcpg_submit_packed_windows.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint32, C.POINTER(WindowSpec), C.POINTER(Params), C.POINTER(vp)]
    L.kmcpg_window_count.argtypes = [vp, C.c_uint32, C.POINTER(WindowSpec), u64p, u64p]
    L.kmcpg_window_locate.argtypes = [vp, C.c_uint32, C.POINTER(WindowSpec), C.c_uint64, C.c_uint64, vp, vp]
    L.kmcpg_density_bins.argtypes = [vp, C.c_uint32, C.POINTER(DensitySpec), u64p]
    L.kmcpg_block_density.argtypes = [vp, C.c_uint32, C.POINTER(DensitySpec), vp, C.c_uint64]
    L.kmcpg_col_ones.argtypes = [vp, vp, C.c_uint64]
    L.kmcpg_last_density_launch.argtypes = [vp, C.POINTER(DensityLaunch)]
    L.kmcpg_last_density_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.kmcpg_stream_probe.argtypes = [vp, C.POINTER(C.c_float), u64p]
    L.kmcpg_open_files.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_int32, C.POINTER(vp)]
    L.kmcpg_sketcher_open.argtypes = [C.POINTER(SketchCfg), C.c_int32, C.POINTER(vp)]
    L.kmcpg_sketcher_close.argtypes = [vp]
    L.kmcpg_split_bounds.argtypes = [C.c_uint64, C.POINTER(SplitSpec), vp, vp, C.c_uint64, u64p]
    L.kmcpg_sketch_genomes.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(SplitSpec), C.POINTER(SketchResult)]
    L.kmcpg_sketch_result_free.argtypes = [C.POINTER(SketchResult)]
    L.kmcpg_sketch_result_free.restype = None
    L.kmcpg_last_sketch_launches.argtypes = [vp, C.POINTER(SketchLaunch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_last_sketch_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.kmcpg_dedup_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.POINTER(DedupSpec), vp]
    L.kmcpg_last_dedup_launches.argtypes = [vp, C.POINTER(DedupLaunch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_sort_segments_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, vp, C.c_uint64, vp,
                                             C.POINTER(SketchLaunch), vp]
    L.kmcpg_open_set.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(Opts), C.POINTER(vp)]
    L.kmcpg_set_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]
    L.kmcpg_last_set_order.argtypes = [vp, C.POINTER(SetOrder)]
    L.kmcpg_set_specific.argtypes = [vp, vp, vp, C.c_uint32]
    L.kmcpg_specific_device.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int32, vp, C.c_uint64, vp, vp, vp]
    L.kmcpg_last_specific.argtypes = [vp, C.POINTER(SpecificStats), C.POINTER(K4Launch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_summarize_device.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp]
    L.kmcpg_last_summary.argtypes = [vp, C.POINTER(SummaryStats), C.POINTER(K4Launch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_submit_windows_summary.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(WindowSpec), C.POINTER(Params), C.POINTER(vp)]
    L.kmcpg_wait_summaries.argtypes = [vp, C.POINTER(ResultSummaries)]
    L.kmcpg_result_summaries_free.argtypes = [C.POINTER(ResultSummaries)]
    L.kmcpg_result_summaries_free.restype = None
    L.kmcpg_set_refstats.argtypes = [vp, vp, vp, C.c_uint32, C.c_double]
    L.kmcpg_refstats_device.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int32, vp, C.c_uint64, vp, vp]
    L.kmcpg_refstats_read.argtypes = [vp, vp, C.c_uint32, C.POINTER(RefstatsTotals)]
    L.kmcpg_refstats_reset.argtypes = [vp]
    L.kmcpg_last_refstats.argtypes = [vp, C.POINTER(RefstatsStats), C.POINTER(K4Launch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_set_cooccur.argtypes = [vp, vp, C.c_uint32, C.c_uint64]
    L.kmcpg_cooccur_device.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int32, vp, C.c_uint64, vp, C.c_uint32, vp]
    L.kmcpg_cooccur_read.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(CooccurTotals)]
    L.kmcpg_cooccur_reset.argtypes = [vp]
    L.kmcpg_last_cooccur.argtypes = [vp, C.POINTER(CooccurStats), C.POINTER(K4Launch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_set_recount.argtypes = [vp, vp, vp, C.c_uint32, C.c_double, C.c_uint64]
    L.kmcpg_recount_log_device.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_int32, vp, C.c_uint64, vp, C.c_uint32, vp]
    L.kmcpg_recount_run.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint64, C.POINTER(RecountParams)]
    L.kmcpg_recount_read.argtypes = [vp, vp, C.c_uint32, C.POINTER(RecountTotals)]
    L.kmcpg_recount_reset.argtypes = [vp]
    L.kmcpg_last_recount.argtypes = [vp, C.POINTER(RecountStats), C.POINTER(K4Launch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_em_pass.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.kmcpg_em_read.argtypes = [vp, vp, C.c_uint32, C.POINTER(EmTotals)]
    L.kmcpg_last_em.argtypes = [vp, C.POINTER(EmStats), C.POINTER(K4Launch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_count_left_reads.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.POINTER(Params), vp, vp, vp]
    L.kmcpg_left_compact_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp]
    L.kmcpg_submit_stats.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.POINTER(Params), C.POINTER(vp)]
    L.kmcpg_wait_stats.argtypes = [vp, C.POINTER(StatsResult)]
    L.kmcpg_last_stats.argtypes = [vp, C.POINTER(StatsTicketStats), C.POINTER(K4Launch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_set_binning.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32]
    L.kmcpg_bin_device.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int32, vp, C.c_uint64, vp, vp]
    L.kmcpg_submit_bins.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.POINTER(Params), C.POINTER(vp)]
    L.kmcpg_wait_bins.argtypes = [vp, vp, C.POINTER(BinsResult)]
    L.kmcpg_last_bins.argtypes = [vp, C.POINTER(BinStats), C.POINTER(K4Launch), C.c_uint32, C.POINTER(C.c_uint32)]
    L.kmcpg_sketch_genomes_to.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(SplitSpec), SKETCH_SINK, vp]
    u32p = C.POINTER(C.c_uint32)
    L.kmcpg_builder_open.argtypes = [C.POINTER(BuilderCfg), C.c_int32, C.POINTER(vp)]
    L.kmcpg_builder_close.argtypes = [vp]
    L.kmcpg_builder_add_cols.argtypes = [vp, C.POINTER(BuildColMeta), C.c_uint32]
    L.kmcpg_builder_plan.argtypes = [vp, C.c_uint64, u32p, u32p]
    L.kmcpg_builder_col_place.argtypes = [vp, C.c_uint32, u32p, u32p, u32p]
    L.kmcpg_builder_block_info.argtypes = [vp, C.c_uint32, u64p, u32p, u32p, u32p]
    L.kmcpg_builder_begin_round.argtypes = [vp, C.c_uint32]
    L.kmcpg_builder_scatter_device.argtypes = [vp, vp, vp, vp, C.c_uint32, vp]
    L.kmcpg_builder_end_round.argtypes = [vp, C.c_char_p]
    L.kmcpg_builder_finish.argtypes = [vp, C.c_char_p]
    L.kmcpg_builder_info.argtypes = [vp, C.POINTER(BuilderStats)]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise KmcpGpuError(rc, load().kmcpg_last_error().decode(errors="replace"))


class Pair(C.Structure):
    _fields_ = [("col", C.c_uint32), ("count", C.c_uint32)]


class ResultPairs(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("k", C.c_int32), ("qlen", C.POINTER(C.c_int32)), ("qkmers", C.POINTER(C.c_int32)),
                ("ksize", C.POINTER(C.c_int32)), ("match_offs", C.POINTER(C.c_uint64)), ("pairs", C.POINTER(Pair)), ("owner", C.c_void_p)]


def window_count(offs, step, window, greedy=False):
    """kmcpg_window_count: (windows, their bases) of the reads of offs[0..n]"""
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    spec = WindowSpec(step, window, 1 if greedy else 0, 0)
    nw, nb = C.c_uint64(), C.c_uint64()
    _check(load().kmcpg_window_count(offs.ctypes.data, len(offs) - 1, C.byref(spec), C.byref(nw), C.byref(nb)))
    return nw.value, nb.value


def window_locate(offs, step, window, greedy=False):
    """kmcpg_window_locate: for every result row of a window batch, the read it came from and the window's 0-based first base"""
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n, _ = window_count(offs, step, window, greedy)
    spec = WindowSpec(step, window, 1 if greedy else 0, 0)
    read = np.zeros(n, dtype=np.uint32)
    start = np.zeros(n, dtype=np.uint64)
    if n:
        _check(load().kmcpg_window_locate(offs.ctypes.data, len(offs) - 1, C.byref(spec), 0, n, read.ctypes.data, start.ctypes.data))
    return read, start


def pack_reads(reads):
    """list of bytes -> (uint8 array, uint64 offsets[n+1])."""
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    if reads:
        offs[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    seqs = np.frombuffer(b"".join(reads), dtype=np.uint8).copy() if reads else np.zeros(0, dtype=np.uint8)
    return seqs, offs


def build_db(out_dir, columns, k=21, num_hashes=1, fpr=0.3, threads=32, block_size=0, scale=1, minimizer_w=0, syncmer_s=0, device=0,
             alias="kmcp-gpu-db", kmers_x=0, block_size_x=0, kmers_8=0, kmers_1=0, uniform_sigs=0):
    """`kmcp index` on the GPU.  columns: list of (name, gsize, chunk_idx, chunks, sorted-unique uint64 hashes).
    uniform_sigs: 0 = the reference's per-block NumSigs; 1 / 2 = blocks share NumSigs (groupable in HBM), see kmcp_gpu.h."""
    cfg = BuildCfg(k=k, canonical=1, num_hashes=num_hashes, fpr=fpr, threads=threads, block_size=block_size, scale=scale,
                   minimizer_w=minimizer_w, syncmer_s=syncmer_s, alias=alias.encode(), kmers_x=kmers_x, block_size_x=block_size_x, kmers_8=kmers_8,
                   kmers_1=kmers_1, uniform_sigs=uniform_sigs)
    arr = (BuildCol * len(columns))()
    keep = []
    for i, (name, gsize, ci, nch, h) in enumerate(columns):
        h = np.ascontiguousarray(h, dtype=np.uint64)
        keep.append(h)
        arr[i] = BuildCol(name.encode(), gsize, ci, nch, h.ctypes.data, len(h))
    _check(load().kmcpg_build_db(os.fsencode(out_dir), C.byref(cfg), arr, len(columns), device))
    return os.path.join(out_dir, "R001")


def copy_from_device(d_ptr, count, dtype=np.uint64, stream=None):
    """`count` items at the device pointer d_ptr (an integer) -> numpy array: a hipMemcpyAsync on `stream` and a wait for that stream,
    through the HIP runtime libkmcpgpu.so is bound to.  What a sketch_to sink uses to look at a piece's lists."""
    out = np.zeros(count, dtype=dtype)
    if count:
        L = load()
        L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.hipStreamSynchronize.argtypes = [C.c_void_p]
        if L.hipMemcpyAsync(out.ctypes.data, d_ptr, out.nbytes, 2, stream) != 0 or L.hipStreamSynchronize(stream) != 0:  # 2 = hipMemcpyDeviceToHost
            raise KmcpGpuError(-4, "copy from the device failed")
    return out


class Builder:
    """kmcpg_builder: `kmcp index` in two passes — the counts of every column first (add_cols, plan), then device-resident lists ORed
    into block matrices that stay in HBM, round by round (begin_round, scatter_device, end_round), then finish.  device=-1 plans only."""

    NO_BLOCK = 0xFFFFFFFF

    def __init__(self, k=21, num_hashes=1, fpr=0.3, threads=32, block_size=0, scale=1, minimizer_w=0, syncmer_s=0, device=0, alias="kmcp-gpu-db",
                 kmers_x=0, block_size_x=0, kmers_8=0, kmers_1=0, uniform_sigs=0, hbm_reserve=0):
        cfg = BuilderCfg()
        cfg.build = BuildCfg(k=k, canonical=1, num_hashes=num_hashes, fpr=fpr, threads=threads, block_size=block_size, scale=scale,
                             minimizer_w=minimizer_w, syncmer_s=syncmer_s, alias=alias.encode(), kmers_x=kmers_x, block_size_x=block_size_x,
                             kmers_8=kmers_8, kmers_1=kmers_1, uniform_sigs=uniform_sigs)
        cfg.hbm_reserve = hbm_reserve
        h = C.c_void_p()
        _check(load().kmcpg_builder_open(C.byref(cfg), device, C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            load().kmcpg_builder_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def add_cols(self, cols):
        """cols: list of (name, gsize, chunk_idx, chunks, n_hashes); input order = column id"""
        arr = (BuildColMeta * max(1, len(cols)))()
        for i, (name, gsize, ci, nch, n) in enumerate(cols):
            arr[i] = BuildColMeta(name.encode(), gsize, ci, nch, n)
        _check(load().kmcpg_builder_add_cols(self._h, arr, len(cols)))

    def plan(self, matrix_budget=0):
        """-> (blocks, rounds)"""
        nb, nr = C.c_uint32(0), C.c_uint32(0)
        _check(load().kmcpg_builder_plan(self._h, matrix_budget, C.byref(nb), C.byref(nr)))
        return nb.value, nr.value

    def col_place(self, col):
        """-> (block, column in the block, round); block NO_BLOCK: an empty column, in no block"""
        b, c, r = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(load().kmcpg_builder_col_place(self._h, col, C.byref(b), C.byref(c), C.byref(r)))
        return b.value, c.value, r.value

    def block_info(self, block):
        ns, n, rb, r = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(load().kmcpg_builder_block_info(self._h, block, C.byref(ns), C.byref(n), C.byref(rb), C.byref(r)))
        return dict(num_sigs=ns.value, n_cols=n.value, row_bytes=rb.value, round=r.value)

    def begin_round(self, rnd):
        _check(load().kmcpg_builder_begin_round(self._h, rnd))

    def scatter_device(self, d_hashes, koff, cols, stream=None):
        """d_hashes: device pointer (integer); koff [n + 1] and cols [n] are host arrays; cols NO_BLOCK = skip the entry"""
        koff = np.ascontiguousarray(koff, dtype=np.uint64)
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        assert len(koff) == len(cols) + 1
        _check(load().kmcpg_builder_scatter_device(self._h, d_hashes, koff.ctypes.data, cols.ctypes.data, len(cols), stream))

    def end_round(self, out_dir):
        _check(load().kmcpg_builder_end_round(self._h, os.fsencode(out_dir)))

    def finish(self, out_dir):
        _check(load().kmcpg_builder_finish(self._h, os.fsencode(out_dir)))
        return os.path.join(out_dir, "R001")

    def info(self):
        st = BuilderStats()
        _check(load().kmcpg_builder_info(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in BuilderStats._fields_ if f != "reserved"}


def split_bounds(length, split_number=1, split_overlap=0, split_min_ref=0, k_min=21, k_max=None):
    """kmcpg_split_bounds: [(first, end), ...] of the chunks `kmcp compute --split-number` cuts a joined sequence of `length` bases into"""
    spec = SplitSpec(split_number, split_overlap, split_min_ref, k_min, k_min if k_max is None else k_max, 0)
    n = C.c_uint64(0)
    _check(load().kmcpg_split_bounds(length, C.byref(spec), None, None, 0, C.byref(n)))
    first = np.zeros(n.value, dtype=np.uint64)
    end = np.zeros(n.value, dtype=np.uint64)
    if n.value:
        _check(load().kmcpg_split_bounds(length, C.byref(spec), first.ctypes.data, end.ctypes.data, n.value, C.byref(n)))
    return [(int(a), int(b)) for a, b in zip(first, end)]


class Sketch:
    """The chunk lists of one Sketcher.sketch call: genome / chunk_idx / chunks per list, and list i = hashes[koff[i]:koff[i + 1]]
    (sorted, unique).  The arrays are views of library memory until close() (or the end of the `with` block)."""

    def __init__(self, res):
        self._res = res
        n = res.n_chunks
        as_np = lambda p, m, dt: np.ctypeslib.as_array(p, shape=(m,)) if m else np.zeros(0, dtype=dt)  # noqa: E731
        self.genome = as_np(res.genome, n, np.uint32)
        self.chunk_idx = as_np(res.chunk_idx, n, np.uint32)
        self.chunks = as_np(res.chunks, n, np.uint32)
        self.koff = np.ctypeslib.as_array(res.koff, shape=(n + 1,))
        self.hashes = as_np(res.hashes, int(self.koff[n]), np.uint64)

    def __len__(self):
        return len(self.genome)

    def list(self, i):
        return self.hashes[int(self.koff[i]):int(self.koff[i + 1])]

    def close(self):
        if self._res is not None:
            self.genome = self.chunk_idx = self.chunks = self.koff = self.hashes = None
            load().kmcpg_sketch_result_free(C.byref(self._res))
            self._res = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Sketcher:
    """kmcpg_sketcher: `kmcp compute` for batches of joined genomes on the GPU."""

    def __init__(self, k=21, scale=1, minimizer_w=0, syncmer_s=0, device=0):
        ks = [k] if isinstance(k, int) else list(k)
        cfg = SketchCfg(n_k=len(ks), scale=scale, minimizer_w=minimizer_w, syncmer_s=syncmer_s)
        for i, v in enumerate(ks[:8]):
            cfg.ks[i] = v
        if len(ks) > 8:
            cfg.n_k = 9  # refused by the library
        self.ks = ks
        h = C.c_void_p()
        _check(load().kmcpg_sketcher_open(C.byref(cfg), device, C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            load().kmcpg_sketcher_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sketch(self, genomes, split_number=1, split_overlap=0, split_min_ref=0):
        """genomes: list of joined sequences (bytes).  Returns a Sketch."""
        seqs, offs = pack_reads(list(genomes))
        spec = SplitSpec(split_number, split_overlap, split_min_ref, min(self.ks), max(self.ks), 0)
        res = SketchResult()
        _check(load().kmcpg_sketch_genomes(self._h, seqs.ctypes.data, offs.ctypes.data, len(genomes), C.byref(spec), C.byref(res)))
        return Sketch(res)

    def sketch_to(self, genomes, sink, split_number=1, split_overlap=0, split_min_ref=0):
        """kmcpg_sketch_genomes_to: sink(piece) is called per piece with a dict of first_chunk, genome / chunk_idx / chunks (numpy copies),
        koff (numpy, n + 1), d_hashes (device pointer as an integer, valid inside the sink only) and stream; it returns None / 0, or an
        error code that ends the call (raised as KmcpGpuError).  An exception in the sink ends the call too and is re-raised."""
        seqs, offs = pack_reads(list(genomes))
        spec = SplitSpec(split_number, split_overlap, split_min_ref, min(self.ks), max(self.ks), 0)
        raised = []

        def tramp(_user, pp):
            try:
                p = pp.contents
                n = p.n_chunks
                arr = lambda ptr, m, dt: np.ctypeslib.as_array(ptr, shape=(m,)).copy() if m else np.zeros(0, dtype=dt)  # noqa: E731
                piece = dict(first_chunk=p.first_chunk, n_chunks=n, genome=arr(p.genome, n, np.uint32), chunk_idx=arr(p.chunk_idx, n, np.uint32),
                             chunks=arr(p.chunks, n, np.uint32), koff=np.ctypeslib.as_array(p.koff, shape=(n + 1,)).copy(),
                             d_hashes=p.d_hashes or 0, stream=p.stream)
                rc = sink(piece)
                return int(rc) if rc else 0
            except BaseException as e:  # nothing may cross the C frames
                raised.append(e)
                return -1

        cb = SKETCH_SINK(tramp)
        rc = load().kmcpg_sketch_genomes_to(self._h, seqs.ctypes.data, offs.ctypes.data, len(genomes), C.byref(spec), cb, None)
        if raised:
            raise raised[0]
        _check(rc)

    def last_sketch_launches(self):
        n = C.c_uint32(0)
        _check(load().kmcpg_last_sketch_launches(self._h, None, 0, C.byref(n)))
        arr = (SketchLaunch * max(1, n.value))()
        _check(load().kmcpg_last_sketch_launches(self._h, arr, n.value, C.byref(n)))
        return [dict(kind=a.kind, passes=a.passes, key_bits=a.key_bits, segments=a.segments, workgroups=a.workgroups, launches=a.launches,
                     keys=a.keys) for a in arr[:n.value]]

    def last_sketch_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        _check(load().kmcpg_last_sketch_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


def last_sketch_launches(sketcher):
    """kmcpg_last_sketch_launches of a Sketcher"""
    return sketcher.last_sketch_launches()


def sort_segments_device(d_keys, d_in_off, d_cnt, part_stride, cnt_stride, parts, n_segs, max_waves, key_bits, d_out, out_cap, d_koff, stream=None):
    """kmcpg_sort_segments_device (debug/tests): the segmented sort + unique on lists laid out in device memory (pointers as integers).
    Returns the launch record as Sketcher.last_sketch_launches gives them."""
    a = SketchLaunch()
    _check(load().kmcpg_sort_segments_device(d_keys, d_in_off, d_cnt, part_stride, cnt_stride, parts, n_segs, max_waves, key_bits, d_out, out_cap,
                                             d_koff, C.byref(a), stream))
    return dict(kind=a.kind, passes=a.passes, key_bits=a.key_bits, segments=a.segments, workgroups=a.workgroups, launches=a.launches, keys=a.keys)


class BatchResult:
    """QueryResult for a batch (numpy copies of kmcpg_result)."""

    def __init__(self, qlen, qkmers, offs, matches, k, ksize=None):
        self.qlen, self.qkmers, self.offs, self.matches, self.k, self.ksize = qlen, qkmers, offs, matches, k, ksize

    def __len__(self):
        return len(self.qlen)

    def read(self, i):
        return self.matches[int(self.offs[i]):int(self.offs[i + 1])]


def _copy_result(r):
    n = r.n_reads
    qlen = np.ctypeslib.as_array(r.qlen, shape=(n,)).copy() if n else np.zeros(0, np.int32)
    qk = np.ctypeslib.as_array(r.qkmers, shape=(n,)).copy() if n else np.zeros(0, np.int32)
    offs = np.ctypeslib.as_array(r.match_offs, shape=(n + 1,)).copy()
    m = int(offs[-1])
    if m:
        buf = C.string_at(r.matches, m * C.sizeof(Match))
        matches = np.frombuffer(buf, dtype=MATCH_DTYPE).copy()
    else:
        matches = np.zeros(0, dtype=MATCH_DTYPE)
    ks = np.ctypeslib.as_array(r.ksize, shape=(n,)).copy() if n else np.zeros(0, np.int32)
    out = BatchResult(qlen, qk, offs, matches, r.k, ks)
    load().kmcpg_result_free(C.byref(r))
    return out


class PairsResult:
    """kmcpg_result_pairs for a batch (numpy copies): the final matches of every query as (column, mKmers) pairs."""

    def __init__(self, qlen, qkmers, offs, pairs, k, ksize):
        self.qlen, self.qkmers, self.offs, self.pairs, self.k, self.ksize = qlen, qkmers, offs, pairs, k, ksize

    def __len__(self):
        return len(self.qlen)

    def read(self, i):
        return self.pairs[int(self.offs[i]):int(self.offs[i + 1])]


def _copy_pairs(r):
    n = r.n_reads
    qlen = np.ctypeslib.as_array(r.qlen, shape=(n,)).copy() if n else np.zeros(0, np.int32)
    qk = np.ctypeslib.as_array(r.qkmers, shape=(n,)).copy() if n else np.zeros(0, np.int32)
    offs = np.ctypeslib.as_array(r.match_offs, shape=(n + 1,)).copy() if n else np.zeros(1, np.uint64)
    ks = np.ctypeslib.as_array(r.ksize, shape=(n,)).copy() if n else np.zeros(0, np.int32)
    m = int(offs[-1])
    pairs = np.frombuffer(C.string_at(r.pairs, m * 8), dtype=np.uint32).reshape(m, 2).copy() if m else np.zeros((0, 2), np.uint32)
    out = PairsResult(qlen, qk, offs, pairs, r.k, ks)
    load().kmcpg_result_pairs_free(C.byref(r))
    return out


class Database:
    """A kmcp database resident in the HBM of one GPU (or one shard of it)."""

    def __init__(self, handle):
        self._h = handle
        info = Info()
        _check(load().kmcpg_db_info(self._h, C.byref(info)))
        self.info = info
        self._names = {}
        n = C.c_int32(0)
        _check(load().kmcpg_db_ks(self._h, None, 0, C.byref(n)))
        buf = (C.c_int32 * max(1, n.value))()
        _check(load().kmcpg_db_ks(self._h, buf, n.value, C.byref(n)))
        self.ks = [int(buf[i]) for i in range(n.value)]  # the database's k-mer sizes, largest first

    @classmethod
    def open(cls, db_dir, device=0, shard_rank=0, shard_count=1):
        h = C.c_void_p()
        o = Opts(device, shard_rank, shard_count, 0)
        _check(load().kmcpg_open(os.fsencode(db_dir), C.byref(o), C.byref(h)))
        return cls(h)

    @classmethod
    def open_set(cls, dirs, device=0):
        """kmcpg_open_set: 1 to 16 database directories as one handle on one GPU; a search returns what kmcp-merge makes of the members'
        separate results (rows by printed score, ties by member, then the member's own order).  device=-1: metadata only."""
        h = C.c_void_p()
        arr = (C.c_char_p * max(1, len(dirs)))(*[os.fsencode(d) for d in dirs])
        o = Opts(device, 0, 1, 0)
        _check(load().kmcpg_open_set(arr, len(dirs), C.byref(o), C.byref(h)))
        return cls(h)

    def set_info(self):
        """kmcpg_set_info: the first global column of every member (one entry for a handle of Database.open)"""
        n = C.c_uint32(0)
        buf = (C.c_uint32 * 16)()
        _check(load().kmcpg_set_info(self._h, C.byref(n), buf, 16))
        return [int(buf[i]) for i in range(min(16, n.value))]

    def last_set_order(self):
        """kmcpg_last_set_order: dict(wave_segments, wg_segments, long_segments, device_mixed_runs, host_segments, host_mixed_runs)"""
        r = SetOrder()
        _check(load().kmcpg_last_set_order(self._h, C.byref(r)))
        return {f: int(getattr(r, f)) for f, _ in SetOrder._fields_}

    @classmethod
    def open_devices(cls, db_dir, devices):
        """One process, several GPUs: blocks partitioned over `devices`, search() fans out and merges on the host."""
        h = C.c_void_p()
        arr = (C.c_int32 * len(devices))(*devices)
        _check(load().kmcpg_open_devices(os.fsencode(db_dir), arr, len(devices), C.byref(h)))
        return cls(h)

    @classmethod
    def open_paged(cls, db_dir, device=0, passes=0):
        """A database larger than the free HBM of one GPU: searched in `passes` shards per batch (0 = as few as fit)."""
        h = C.c_void_p()
        _check(load().kmcpg_open_paged(os.fsencode(db_dir), device, passes, C.byref(h)))
        return cls(h)

    @classmethod
    def open_files(cls, paths, device=0):
        """kmcpg_open_files: a handle over the given .uniki files alone (no __db.yml), blocks numbered in argument order; index
        inspection and row read-back only, every search entry point refuses.  device=-1: headers only."""
        h = C.c_void_p()
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        _check(load().kmcpg_open_files(arr, len(paths), device, C.byref(h)))
        return cls(h)

    # ---- index inspection (kmcp utils index-density / ref-info) -------------------------------------------------
    def density_bins(self, block, bin_rows, first_row=0, n_rows=0, reserved=0):
        """kmcpg_density_bins: bins of a request (the last one may be short)"""
        spec = DensitySpec(bin_rows, first_row, n_rows, reserved)
        n = C.c_uint64(0)
        _check(load().kmcpg_density_bins(self._h, block, C.byref(spec), C.byref(n)))
        return int(n.value)

    def block_density(self, block, bin_rows, first_row=0, n_rows=0):
        """kmcpg_block_density: set bits per (column of the block, bin of bin_rows rows) -> uint32 [n_cols, n_bins]"""
        n_bins = self.density_bins(block, bin_rows, first_row, n_rows)
        n_cols = self.block_info(block)["n_cols"]
        out = np.zeros((n_cols, n_bins), dtype=np.uint32)
        spec = DensitySpec(bin_rows, first_row, n_rows, 0)
        _check(load().kmcpg_block_density(self._h, block, C.byref(spec), out.ctypes.data, out.size))
        return out

    def col_ones(self):
        """kmcpg_col_ones: set bits of every global column over all its rows (0 for columns of non-local blocks) -> uint64 [n_cols]"""
        out = np.zeros(int(self.info.n_cols), dtype=np.uint64)
        _check(load().kmcpg_col_ones(self._h, out.ctypes.data, out.size))
        return out

    def last_density_launch(self):
        """what the last block_density / col_ones call launched: dict(form "csa" | "small", lpr, npl, workgroups, launches)"""
        r = DensityLaunch()
        _check(load().kmcpg_last_density_launch(self._h, C.byref(r)))
        return dict(form=DENSITY_FORMS[r.form], lpr=r.lpr, npl=r.npl, workgroups=r.workgroups, launches=r.launches)

    def last_density_ms(self):
        """HIP-event milliseconds of the device work of the last block_density / col_ones call"""
        ms = C.c_float()
        _check(load().kmcpg_last_density_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def stream_probe(self):
        """kmcpg_stream_probe: (ms, bytes) of one read-only pass over every resident group's rows, 16 B per lane and one XOR per load"""
        ms, n = C.c_float(), C.c_uint64()
        _check(load().kmcpg_stream_probe(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def save(self, out_dir):
        """kmcpg_save_db: the resident database as <out_dir>/R001 in the reference's on-disk format; returns that directory."""
        _check(load().kmcpg_save_db(self._h, os.fsencode(out_dir)))
        return os.path.join(out_dir, "R001")

    def exchange_info(self):
        return load().kmcpg_exchange_info(self._h).decode()

    def paged_info(self):
        """(passes, shard uploads so far); passes == 0 for resident handles"""
        p, u = C.c_int32(0), C.c_uint64(0)
        _check(load().kmcpg_paged_info(self._h, C.byref(p), C.byref(u)))
        return int(p.value), int(u.value)

    def batch_hint(self):
        """bases one batch may hold so that its device workspace fits beside the resident index (0 = unknown)"""
        n = C.c_uint64(0)
        _check(load().kmcpg_batch_hint(self._h, C.byref(n)))
        return int(n.value)

    @classmethod
    def open_synthetic(cls, spec: SynthSpec, device=0, shard_rank=0, shard_count=1):
        h = C.c_void_p()
        o = Opts(device, shard_rank, shard_count, 0)
        _check(load().kmcpg_open_synthetic(C.byref(spec), C.byref(o), C.byref(h)))
        return cls(h)

    def close(self):
        if self._h:
            load().kmcpg_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def col_info(self, col):
        if col not in self._names:
            name, ti, gs, sz = C.c_char_p(), C.c_uint32(), C.c_uint64(), C.c_uint64()
            _check(load().kmcpg_col_info(self._h, col, C.byref(name), C.byref(ti), C.byref(gs), C.byref(sz)))
            self._names[col] = (name.value.decode(), ti.value, gs.value, sz.value)
        return self._names[col]

    def block_info(self, b):
        ns, nc, rb, st, loc, cb = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int32(), C.c_uint32()
        _check(load().kmcpg_block_info(self._h, b, C.byref(ns), C.byref(nc), C.byref(rb), C.byref(st), C.byref(loc), C.byref(cb)))
        return dict(num_sigs=ns.value, n_cols=nc.value, row_bytes=rb.value, stride=st.value, local=bool(loc.value), col_base=cb.value)

    # ---- whole pipeline, host buffers -------------------------------------------------------------
    def search(self, reads, reads2=None, params=None):
        seqs, offs = pack_reads(reads)
        s2 = o2 = None
        if reads2 is not None:
            s2, o2 = pack_reads(reads2)
        return self.search_packed(seqs, offs, s2, o2, params)

    def search_packed(self, seqs, offs, seqs2=None, offs2=None, params=None):
        p = params or default_params()
        r = Result()
        n = len(offs) - 1
        _check(load().kmcpg_search_batch(self._h, seqs.ctypes.data, offs.ctypes.data,
                                         seqs2.ctypes.data if seqs2 is not None else None,
                                         offs2.ctypes.data if offs2 is not None else None, n, C.byref(p), C.byref(r)))
        return _copy_result(r)

    def submit(self, seqs, offs, seqs2=None, offs2=None, params=None):
        """kmcpg_submit: returns a ticket; the arrays may be reused at once."""
        p = params or default_params()
        t = C.c_void_p()
        n = len(offs) - 1
        _check(load().kmcpg_submit(self._h, seqs.ctypes.data, offs.ctypes.data, seqs2.ctypes.data if seqs2 is not None else None,
                                   offs2.ctypes.data if offs2 is not None else None, n, C.byref(p), C.byref(t)))
        return t

    def submit_packed(self, codes, offs, exc, params=None):
        """kmcpg_submit_packed: a batch as 2-bit codes (pack2) + exception runs; offs in bases."""
        p = params or default_params()
        t = C.c_void_p()
        n = len(offs) - 1
        _check(load().kmcpg_submit_packed(self._h, codes.ctypes.data, offs.ctypes.data, exc.ctypes.data if len(exc) else None, len(exc), n, C.byref(p), C.byref(t)))
        return t

    # ---- sliding windows of long queries (seqkit sliding -s step -W window [-g] | kmcp search) -----------------
    def submit_windows(self, seqs, offs, step, window, greedy=False, params=None):
        """kmcpg_submit_windows: one result row per window (wait / wait_pairs); single-end reads as text + offsets"""
        p = params or default_params()
        spec = WindowSpec(step, window, 1 if greedy else 0, 0)
        t = C.c_void_p()
        n = len(offs) - 1
        _check(load().kmcpg_submit_windows(self._h, seqs.ctypes.data, offs.ctypes.data, n, C.byref(spec), C.byref(p), C.byref(t)))
        return t

    def submit_packed_windows(self, codes, offs, exc, step, window, greedy=False, params=None):
        """kmcpg_submit_packed_windows: the same on reads as 2-bit codes (pack2) + exception runs"""
        p = params or default_params()
        spec = WindowSpec(step, window, 1 if greedy else 0, 0)
        t = C.c_void_p()
        n = len(offs) - 1
        _check(load().kmcpg_submit_packed_windows(self._h, codes.ctypes.data, offs.ctypes.data, exc.ctypes.data if len(exc) else None, len(exc), n,
                                                  C.byref(spec), C.byref(p), C.byref(t)))
        return t

    def search_windows(self, reads, step, window, greedy=False, params=None, pairs=False):
        """windows of `reads` (list of bytes) searched as queries -> (BatchResult or PairsResult, read of each row, start of each row)"""
        seqs, offs = pack_reads(reads)
        t = self.submit_windows(seqs, offs, step, window, greedy, params)
        res = self.wait_pairs(t) if pairs else self.wait(t)
        return (res,) + window_locate(offs, step, window, greedy)

    def search_packed_windows(self, codes, offs, exc, step, window, greedy=False, params=None, pairs=False):
        """the same on a batch as 2-bit codes + exception runs (pack2); offs in bases"""
        t = self.submit_packed_windows(codes, offs, exc, step, window, greedy, params)
        res = self.wait_pairs(t) if pairs else self.wait(t)
        return (res,) + window_locate(offs, step, window, greedy)

    def wait(self, ticket, count_only=False):
        """kmcpg_wait: the finalized matches of a submitted batch (or just their number)."""
        r = Result()
        _check(load().kmcpg_wait(ticket, C.byref(r)))
        if count_only:
            m = int(r.match_offs[r.n_reads])
            load().kmcpg_result_free(C.byref(r))
            return m
        return _copy_result(r)

    # ---- compact results: (column, mKmers) pairs instead of Match records ------------------------
    def search_pairs(self, reads, reads2=None, params=None):
        seqs, offs = pack_reads(reads)
        s2 = o2 = None
        if reads2 is not None:
            s2, o2 = pack_reads(reads2)
        return self.search_packed_pairs(seqs, offs, s2, o2, params)

    def search_packed_pairs(self, seqs, offs, seqs2=None, offs2=None, params=None, count_only=False):
        p = params or default_params()
        r = ResultPairs()
        n = len(offs) - 1
        _check(load().kmcpg_search_batch_pairs(self._h, seqs.ctypes.data, offs.ctypes.data, seqs2.ctypes.data if seqs2 is not None else None,
                                               offs2.ctypes.data if offs2 is not None else None, n, C.byref(p), C.byref(r)))
        if count_only:
            m = int(r.match_offs[n]) if n else 0
            load().kmcpg_result_pairs_free(C.byref(r))
            return m
        return _copy_pairs(r)

    def wait_pairs(self, ticket, count_only=False):
        r = ResultPairs()
        _check(load().kmcpg_wait_pairs(ticket, C.byref(r)))
        if count_only:
            m = int(r.match_offs[r.n_reads]) if r.n_reads else 0
            load().kmcpg_result_pairs_free(C.byref(r))
            return m
        return _copy_pairs(r)

    def expand_pairs(self, qkmers, pairs):
        """kmcpg_expand_pairs: the Match records (MATCH_DTYPE) of one query's pairs"""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        out = np.zeros(len(pairs), dtype=MATCH_DTYPE)
        _check(load().kmcpg_expand_pairs(self._h, int(qkmers), pairs.ctypes.data, len(pairs), out.ctypes.data))
        return out

    def search_packed_count(self, seqs, offs, params=None):
        """kmcpg_search_batch without copying the result into numpy: returns the number of matches (timing of the C boundary)."""
        p = params or default_params()
        r = Result()
        n = len(offs) - 1
        _check(load().kmcpg_search_batch(self._h, seqs.ctypes.data, offs.ctypes.data, None, None, n, C.byref(p), C.byref(r)))
        m = int(r.match_offs[n])
        load().kmcpg_result_free(C.byref(r))
        return m

    # ---- GPU half on device pointers (torch tensors' data_ptr()) ----------------------------------
    def query_device(self, d_seqs, d_offs, n_reads, total_bases, max_read_len, d_hits, hit_cap, d_counters, d_qkmers,
                     d_qlen, params=None, d_seqs2=None, d_offs2=None, stream=None):
        p = params or default_params()
        _check(load().kmcpg_query_device(self._h, d_seqs, d_offs, d_seqs2, d_offs2, n_reads, total_bases, max_read_len,
                                         C.byref(p), d_hits, hit_cap, d_counters, d_qkmers, d_qlen, stream))

    def kmers_device(self, d_seqs, d_offs, n_reads, total_bases, max_read_len, d_hashes, hashes_cap, d_koff, d_nk,
                     params=None, stream=None):
        p = params or default_params()
        _check(load().kmcpg_kmers_device(self._h, d_seqs, d_offs, n_reads, total_bases, max_read_len, C.byref(p),
                                         d_hashes, hashes_cap, d_koff, d_nk, stream))

    def kmers_device_packed(self, d_codes, d_exc, n_exc, d_text, d_offs, n_reads, total_bases, max_read_len, d_hashes, hashes_cap, d_koff, d_nk,
                            params=None, stream=None):
        """kmers_device on a batch that is on the device as 2-bit codes + runs of foreign bytes (kmcpg_kmers_device_packed)"""
        p = params or default_params()
        _check(load().kmcpg_kmers_device_packed(self._h, d_codes, d_exc, n_exc, d_text, d_offs, n_reads, total_bases, max_read_len, C.byref(p),
                                                d_hashes, hashes_cap, d_koff, d_nk, stream))

    def kmers_device_paired(self, d_seqs, d_offs, d_seqs2, d_offs2, n_reads, total_bases, max_read_len, d_hashes, hashes_cap, d_nk, d_nk1=None,
                            params=None, stream=None):
        """kmers_device on pairs (kmcpg_kmers_device_paired): total_bases over both mates; the hashes of pair i (mate 1's, then mate 2's)
        start at offs[i] + offs2[i]; d_nk1 receives the first mate's count"""
        p = params or default_params()
        _check(load().kmcpg_kmers_device_paired(self._h, d_seqs, d_offs, d_seqs2, d_offs2, n_reads, total_bases, max_read_len, C.byref(p),
                                                d_hashes, hashes_cap, d_nk, d_nk1, stream))

    def kmers_device_windows(self, d_text, d_soffs, d_wpre, d_vpre, d_cpre, n_slices, staged_bases, n_chunks, n_windows, window_bases,
                             max_window_len, spec, d_hashes, hashes_cap, d_koff, d_src, d_nk, d_qlen, params=None, stream=None):
        """the k-mer stage alone on a staged piece of sliding windows, as a lane runs it (kmcpg_kmers_device_windows): the slices' text
        (16 readable bytes behind it) and their four prefix arrays [n_slices + 1] in, per window the hashes at d_hashes[d_koff[w] ...],
        d_src, d_nk and d_qlen out; spec = WindowSpec(step, window, greedy, 0)"""
        p = params or default_params()
        _check(load().kmcpg_kmers_device_windows(self._h, d_text, d_soffs, d_wpre, d_vpre, d_cpre, n_slices, staged_bases, n_chunks, n_windows,
                                                 window_bases, max_window_len, C.byref(spec), C.byref(p), d_hashes, hashes_cap, d_koff, d_src,
                                                 d_nk, d_qlen, stream))

    def _k1_records(self):
        n = C.c_uint32(0)
        _check(load().kmcpg_last_k1_launches(self._h, None, 0, C.byref(n)))
        buf = (K1Launch * max(1, n.value))()
        _check(load().kmcpg_last_k1_launches(self._h, buf, n.value, C.byref(n)))
        return list(buf[:n.value])

    def last_k1_launches(self):
        """The K1 kernels the handle's last k-mer stage launched, in launch order (profiling level >= 1, [] without): tuples
        (kernel, p0, p1, grid, block, lds_bytes) with kernel in K1_KERNELS[1:]; p0 / p1 are the kernel's template parameters (MODE, or
        WSZ and WAVES of k1_windows_roll), 0 where it has none."""
        return [(K1_KERNELS[r.kernel], r.p0, r.p1, r.grid, r.block, r.lds_bytes) for r in self._k1_records() if r.kernel != 0]

    def last_k1_plan(self):
        """The plan of that stage (k1_plan.hpp): dict(form in K1_FORMS, codes_direct, list_fallback, adj_done, left_on_list) or None without
        profiling.  left_on_list: what the first kernel of a list form left to the kernel behind it; None = no list, or not read (only
        kmers_device* read it back)."""
        for r in self._k1_records():
            if r.kernel == 0:
                return dict(form=K1_FORMS[r.p0], codes_direct=bool(r.p1 & 1), list_fallback=bool(r.p1 & 2), adj_done=bool(r.p1 & 4),
                            left_on_list=None if r.left_on_list == 0xFFFFFFFF else int(r.left_on_list))
        return None

    def dedup_device(self, d_hashes, d_scratch, d_offs, d_offs2, d_nk_raw, d_nk_search, n_reads, max_n, dedup_threshold, min_matched=1, pre=0,
                     pre_done=0, key_shift=0, stream=None):
        """kmcpg_dedup_device (debug/tests): the dedup stage of the k-mer step alone on hash lists laid out in device memory (pointers as
        integers; d_offs2 may be None).  Enqueues; the caller synchronises."""
        spec = DedupSpec(dedup_threshold, min_matched, pre, pre_done, key_shift)
        _check(load().kmcpg_dedup_device(self._h, d_hashes, d_scratch, d_offs, d_offs2, d_nk_raw, d_nk_search, n_reads, max_n, C.byref(spec), stream))

    def last_dedup_launches(self):
        """What the handle's last dedup stage launched, in launch order (profiling level >= 1, [] without): tuples
        (kernel, p0, p1, p2, grid, block, lo, hi) with kernel in DEDUP_KERNELS; the first names the branch (launch_dedup or k_nk_simple)."""
        n = C.c_uint32(0)
        _check(load().kmcpg_last_dedup_launches(self._h, None, 0, C.byref(n)))
        buf = (DedupLaunch * max(1, n.value))()
        _check(load().kmcpg_last_dedup_launches(self._h, buf, n.value, C.byref(n)))
        return [(DEDUP_KERNELS[r.kernel], r.p0, r.p1, r.p2, r.grid, r.block, r.lo, r.hi) for r in buf[:n.value]]

    def k1_codes_batches(self):
        """(packed batches whose k-mer kernels read the codes directly, packed batches expanded to text first)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(load().kmcpg_k1_codes_batches(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def finalize(self, hits, qkmers, qlen, params=None):
        """hits: structured array HIT_DTYPE (any order, may be the concatenation of all shards)."""
        p = params or default_params()
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        qkmers = np.ascontiguousarray(qkmers, dtype=np.int32)
        qlen = np.ascontiguousarray(qlen, dtype=np.int32)
        r = Result()
        _check(load().kmcpg_finalize(self._h, hits.ctypes.data, len(hits), qkmers.ctypes.data, qlen.ctypes.data,
                                     len(qkmers), C.byref(p), C.byref(r)))
        return _copy_result(r)

    def finalize_count(self, hits_u32, qkmers, qlen, params=None):
        """kmcpg_finalize on raw buffers (hits: C-contiguous int32/uint32 [n, 3]); returns the number of matches, copies nothing."""
        p = params or default_params()
        assert hits_u32.flags["C_CONTIGUOUS"] and hits_u32.dtype.itemsize == 4 and qkmers.dtype == np.int32 and qlen.dtype == np.int32
        r = Result()
        n = len(qkmers)
        _check(load().kmcpg_finalize(self._h, hits_u32.ctypes.data, hits_u32.shape[0], qkmers.ctypes.data, qlen.ctypes.data, n, C.byref(p), C.byref(r)))
        m = int(r.match_offs[n]) if n else 0
        load().kmcpg_result_free(C.byref(r))
        return m

    # ---- the host half split in two: K3 on the device (group, -T, order), expansion to Match records on the host ----------
    def group_device(self, d_hits, d_n_hits, hit_cap, d_qkmers, n_reads, d_pairs, d_read_offs, params=None, stream=None):
        """kmcpg_group_device on device pointers: hits as query_device left them -> (column, count) pairs grouped by read, filtered by
        -T, ordered per read; d_read_offs needs n_reads + 2 uint64 words."""
        p = params or default_params()
        _check(load().kmcpg_group_device(self._h, d_hits, d_n_hits, hit_cap, d_qkmers, n_reads, C.byref(p), d_pairs, d_read_offs, stream))

    # ---- species-specific queries: K4 behind K3 ----------------------------------------------------------------
    def set_specific(self, target_class=None, species_class=None):
        """kmcpg_set_specific: one uint32 per global column each; species_class None = strain / assembly level; no argument = off."""
        if target_class is None:
            assert species_class is None
            _check(load().kmcpg_set_specific(self._h, None, None, 0))
            return
        t = np.ascontiguousarray(target_class, dtype=np.uint32)
        s = None if species_class is None else np.ascontiguousarray(species_class, dtype=np.uint32)
        assert s is None or len(s) == len(t)
        _check(load().kmcpg_set_specific(self._h, t.ctypes.data, None if s is None else s.ctypes.data, len(t)))

    def specific_device(self, d_pairs, d_read_offs, pair_cap, d_qkmers, n_reads, final_n, d_out_pairs, out_cap, d_out_offs, d_verdicts, stream=None):
        """kmcpg_specific_device on device pointers: K3's pairs and offsets -> a verdict byte per read, the surviving segments and
        their offsets (n_reads + 1 words)."""
        _check(load().kmcpg_specific_device(self._h, d_pairs, d_read_offs, pair_cap, d_qkmers, n_reads, final_n, d_out_pairs, out_cap, d_out_offs,
                                            d_verdicts, stream))

    def last_specific(self):
        """kmcpg_last_specific: (dict of the counters, [K4Launch] of the last K4 launch — empty below profiling level 1)"""
        st = SpecificStats()
        n = C.c_uint32(0)
        _check(load().kmcpg_last_specific(self._h, C.byref(st), None, 0, C.byref(n)))
        buf = (K4Launch * max(1, n.value))()
        _check(load().kmcpg_last_specific(self._h, C.byref(st), buf, n.value, C.byref(n)))
        self.last_k4_ms = float(st.k4_ms)  # HIP-event time of the stage's kernels (profiling level >= 1), else -1
        return {f: int(getattr(st, f)) for f, _ in SpecificStats._fields_ if f != "k4_ms"}, [buf[i] for i in range(n.value)]

    # ---- reference statistics: K6 behind K3 ---------------------------------------------------------------------
    def set_refstats(self, target_class=None, species_class=None, hic_min_qcov=0.75):
        """kmcpg_set_refstats: one uint32 per global column each; species_class None = strain / assembly level; no argument = off."""
        if target_class is None:
            assert species_class is None
            _check(load().kmcpg_set_refstats(self._h, None, None, 0, 0.0))
            return
        t = np.ascontiguousarray(target_class, dtype=np.uint32)
        s = None if species_class is None else np.ascontiguousarray(species_class, dtype=np.uint32)
        assert s is None or len(s) == len(t)
        _check(load().kmcpg_set_refstats(self._h, t.ctypes.data, None if s is None else s.ctypes.data, len(t), float(hic_min_qcov)))

    def refstats_device(self, d_pairs, d_read_offs, pair_cap, d_qkmers, n_reads, final_n, d_left, d_n_hits=None, hit_cap=0, stream=None):
        """kmcpg_refstats_device on device pointers: K3's pairs and offsets -> the handle's counters and a LEFT byte per read."""
        _check(load().kmcpg_refstats_device(self._h, d_pairs, d_read_offs, pair_cap, d_qkmers, n_reads, final_n, d_n_hits, hit_cap, d_left, stream))

    def refstats_read(self, n_cols):
        """kmcpg_refstats_read: (COL_STATS_DTYPE [n_cols], dict of the totals) — device and host counters added"""
        out = np.zeros(n_cols, dtype=COL_STATS_DTYPE)
        tot = RefstatsTotals()
        _check(load().kmcpg_refstats_read(self._h, out.ctypes.data, n_cols, C.byref(tot)))
        return out, {f: int(getattr(tot, f)) for f, _ in RefstatsTotals._fields_}

    def refstats_reset(self):
        _check(load().kmcpg_refstats_reset(self._h))

    def last_refstats(self):
        """kmcpg_last_refstats: (dict of the counters, [K4Launch] of the last K6 launch — empty below profiling level 1)"""
        st = RefstatsStats()
        n = C.c_uint32(0)
        _check(load().kmcpg_last_refstats(self._h, C.byref(st), None, 0, C.byref(n)))
        buf = (K4Launch * max(1, n.value))()
        _check(load().kmcpg_last_refstats(self._h, C.byref(st), buf, n.value, C.byref(n)))
        self.last_k6_ms = float(st.k6_ms)  # HIP-event time of the kernel (profiling level >= 1), else -1
        return {f: int(getattr(st, f)) for f, _ in RefstatsStats._fields_ if f != "k6_ms"}, [buf[i] for i in range(n.value)]

    # ---- shared reads of reference pairs: K7 behind K3 -----------------------------------------------------------
    def set_cooccur(self, target_class=None, table_slots=0):
        """kmcpg_set_cooccur: one uint32 per global column; table_slots a power of two (0 = the default); no argument = off."""
        if target_class is None:
            _check(load().kmcpg_set_cooccur(self._h, None, 0, 0))
            return
        t = np.ascontiguousarray(target_class, dtype=np.uint32)
        _check(load().kmcpg_set_cooccur(self._h, t.ctypes.data, len(t), int(table_slots)))

    def cooccur_device(self, d_pairs, d_read_offs, pair_cap, d_qkmers, n_reads, final_n, d_left, d_n_hits=None, hit_cap=0, max_wgs=0, stream=None):
        """kmcpg_cooccur_device on device pointers: K3's pairs and offsets -> the handle's pair table and a LEFT byte per read."""
        _check(load().kmcpg_cooccur_device(self._h, d_pairs, d_read_offs, pair_cap, d_qkmers, n_reads, final_n, d_n_hits, hit_cap, d_left, max_wgs, stream))

    def cooccur_read(self):
        """kmcpg_cooccur_read: (COOCCUR_DTYPE [n_pairs] sorted by (class_a, class_b), dict of the totals) — device table and host map merged"""
        tot = CooccurTotals()
        n = C.c_uint64(0)
        _check(load().kmcpg_cooccur_read(self._h, None, 0, C.byref(n), C.byref(tot)))
        out = np.zeros(n.value, dtype=COOCCUR_DTYPE)
        _check(load().kmcpg_cooccur_read(self._h, out.ctypes.data if n.value else None, n.value, C.byref(n), C.byref(tot)))
        return out[:n.value], {f: int(getattr(tot, f)) for f, _ in CooccurTotals._fields_}

    def cooccur_reset(self):
        _check(load().kmcpg_cooccur_reset(self._h))

    def last_cooccur(self):
        """kmcpg_last_cooccur: (dict of the counters, [K4Launch] of the last K7 launch — empty below profiling level 1)"""
        st = CooccurStats()
        n = C.c_uint32(0)
        _check(load().kmcpg_last_cooccur(self._h, C.byref(st), None, 0, C.byref(n)))
        buf = (K4Launch * max(1, n.value))()
        _check(load().kmcpg_last_cooccur(self._h, C.byref(st), buf, n.value, C.byref(n)))
        self.last_k7_ms = float(st.k7_ms)  # HIP-event time of the kernel (profiling level >= 1), else -1
        return {f: int(getattr(st, f)) for f, _ in CooccurStats._fields_ if f != "k7_ms"}, [buf[i] for i in range(n.value)]

    # ---- recount with ambiguity correction: K8, a log kernel behind K3 and a replay after the last batch ---------
    def set_recount(self, target_class=None, species_class=None, hic_min_qcov=0.75, log_bytes=0):
        """kmcpg_set_recount: one uint32 per global column each (species_class None: strain / assembly level); log_bytes: the read log in
        device memory (0 = the default); no argument = off."""
        if target_class is None:
            _check(load().kmcpg_set_recount(self._h, None, None, 0, 0.0, 0))
            self._n_recount_cols = 0
            return
        t = np.ascontiguousarray(target_class, dtype=np.uint32)
        s = None if species_class is None else np.ascontiguousarray(species_class, dtype=np.uint32)
        if s is not None and len(s) != len(t):
            raise ValueError("target_class and species_class differ in length")
        _check(load().kmcpg_set_recount(self._h, t.ctypes.data, None if s is None else s.ctypes.data, len(t), float(hic_min_qcov), int(log_bytes)))
        self._n_recount_cols = len(t)

    def recount_log_device(self, d_pairs, d_read_offs, pair_cap, d_qkmers, d_qlen, n_reads, final_n, d_left, d_n_hits=None, hit_cap=0, max_wgs=0, stream=None):
        """kmcpg_recount_log_device on device pointers: K3's pairs and offsets -> the single-target counters, the read log and a LEFT byte per read."""
        _check(load().kmcpg_recount_log_device(self._h, d_pairs, d_read_offs, pair_cap, d_qkmers, d_qlen, n_reads, final_n, d_n_hits, hit_cap, d_left, max_wgs, stream))

    def recount_run(self, classes, pairs, min_dreads_prop=0.05, max_mismatch_err=0.05, no_amb_corr=False, level_species=True):
        """kmcpg_recount_run: classes RECOUNT_CLASS_DTYPE [n_classes] (kept, reads, ureads of stage 1), pairs COOCCUR_DTYPE as cooccur_read
        returns them; replays the logs (they are kept: the call can be repeated with other arguments)."""
        c = np.ascontiguousarray(classes, dtype=RECOUNT_CLASS_DTYPE)
        p = np.ascontiguousarray(pairs, dtype=COOCCUR_DTYPE)
        par = RecountParams(1 - float(min_dreads_prop), float(max_mismatch_err), int(bool(no_amb_corr)), int(bool(level_species)))
        _check(load().kmcpg_recount_run(self._h, c.ctypes.data if len(c) else None, len(c), p.ctypes.data if len(p) else None, len(p), C.byref(par)))

    def recount_read(self):
        """kmcpg_recount_read: (RECOUNT_DTYPE [n_cols] in units, dict of the totals) — single-target reads + device replay + host replay"""
        n = getattr(self, "_n_recount_cols", 0)
        out = np.zeros(n, dtype=RECOUNT_DTYPE)
        tot = RecountTotals()
        _check(load().kmcpg_recount_read(self._h, out.ctypes.data if n else None, n, C.byref(tot)))
        return out, {f: int(getattr(tot, f)) for f, _ in RecountTotals._fields_}

    def recount_reset(self):
        _check(load().kmcpg_recount_reset(self._h))

    def last_recount(self):
        """kmcpg_last_recount: (dict of the counters, [K4Launch] of the last k8_log launch and the last replay — empty below profiling level 1)"""
        st = RecountStats()
        n = C.c_uint32(0)
        _check(load().kmcpg_last_recount(self._h, C.byref(st), None, 0, C.byref(n)))
        buf = (K4Launch * max(1, n.value))()
        _check(load().kmcpg_last_recount(self._h, C.byref(st), buf, n.value, C.byref(n)))
        self.last_k8_log_ms, self.last_k8_replay_ms = float(st.log_ms), float(st.replay_ms)
        return {f: int(getattr(st, f)) for f, _ in RecountStats._fields_ if f not in ("log_ms", "replay_ms", "reserved")}, [buf[i] for i in range(n.value)]

    # ---- abundance estimation by EM: K9, a pass over the logs the recount stage keeps ------------------------------
    def em_pass(self, classes, level_species=True):
        """kmcpg_em_pass: classes EM_CLASS_DTYPE [n_classes] (est, coverage); one pass over the device log and the host log (they are kept:
        the call can be repeated with other classes)."""
        c = np.ascontiguousarray(classes, dtype=EM_CLASS_DTYPE)
        _check(load().kmcpg_em_pass(self._h, c.ctypes.data if len(c) else None, len(c), int(bool(level_species))))

    def em_read(self):
        """kmcpg_em_read: (EM_COL_DTYPE [n_cols], dict of the totals) — single-target reads of estimated classes + both halves of the pass"""
        n = getattr(self, "_n_recount_cols", 0)
        out = np.zeros(n, dtype=EM_COL_DTYPE)
        tot = EmTotals()
        _check(load().kmcpg_em_read(self._h, out.ctypes.data if n else None, n, C.byref(tot)))
        return out, {f: int(getattr(tot, f)) for f, _ in EmTotals._fields_}

    def last_em(self):
        """kmcpg_last_em: (dict of the counters, [K4Launch] of the last k9_em launch — empty below profiling level 1)"""
        st = EmStats()
        n = C.c_uint32(0)
        _check(load().kmcpg_last_em(self._h, C.byref(st), None, 0, C.byref(n)))
        buf = (K4Launch * max(1, n.value))()
        _check(load().kmcpg_last_em(self._h, C.byref(st), buf, n.value, C.byref(n)))
        self.last_k9_ms = float(st.em_ms)
        return {f: int(getattr(st, f)) for f, _ in EmStats._fields_ if f != "em_ms"}, [buf[i] for i in range(n.value)]

    # ---- window summaries for region merging: K5 behind K4 ------------------------------------------------------
    def summarize_device(self, d_pairs, d_offs, pair_cap, d_verdicts, d_qkmers, n, d_out, d_left_pairs, left_cap, d_left_offs, stream=None):
        """kmcpg_summarize_device on device pointers: K4's surviving segments -> one 16-byte record per window (SUMMARY_DTYPE), the pairs of
        the windows LEFT to the host compacted behind d_left_pairs with their offsets (n + 1 words)."""
        _check(load().kmcpg_summarize_device(self._h, d_pairs, d_offs, pair_cap, d_verdicts, d_qkmers, n, d_out, d_left_pairs, left_cap, d_left_offs, stream))

    def last_summary(self):
        """kmcpg_last_summary: (dict of the counters, [K4Launch] of the last K5 launch — empty below profiling level 1)"""
        st = SummaryStats()
        n = C.c_uint32(0)
        _check(load().kmcpg_last_summary(self._h, C.byref(st), None, 0, C.byref(n)))
        buf = (K4Launch * max(1, n.value))()
        _check(load().kmcpg_last_summary(self._h, C.byref(st), buf, n.value, C.byref(n)))
        self.last_k5_ms = float(st.k5_ms)  # HIP-event time of the stage's kernels (profiling level >= 1), else -1
        return {f: int(getattr(st, f)) for f, _ in SummaryStats._fields_ if f != "k5_ms"}, [buf[i] for i in range(n.value)]

    def submit_windows_summary(self, seqs, offs, step, window, greedy=False, params=None):
        """kmcpg_submit_windows_summary: submit_windows with the species-specific stage on and K5 behind it (wait_summaries)"""
        p = params or default_params()
        spec = WindowSpec(step, window, 1 if greedy else 0, 0)
        t = C.c_void_p()
        n = len(offs) - 1
        _check(load().kmcpg_submit_windows_summary(self._h, seqs.ctypes.data, offs.ctypes.data, n, C.byref(spec), C.byref(p), C.byref(t)))
        return t

    def wait_summaries(self, ticket):
        """kmcpg_wait_summaries: (summaries SUMMARY_DTYPE [n_windows], qlen int32, qkmers int32)"""
        r = ResultSummaries()
        _check(load().kmcpg_wait_summaries(ticket, C.byref(r)))
        n = int(r.n_windows)
        try:
            if n == 0:
                return np.zeros(0, dtype=SUMMARY_DTYPE), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
            s = np.frombuffer(C.string_at(r.s, n * C.sizeof(WindowSummary)), dtype=SUMMARY_DTYPE).copy()
            return s, np.ctypeslib.as_array(r.qlen, shape=(n,)).copy(), np.ctypeslib.as_array(r.qkmers, shape=(n,)).copy()
        finally:
            load().kmcpg_result_summaries_free(C.byref(r))

    def finalize_grouped(self, pairs, read_offs, qkmers, qlen, params=None, count_only=False):
        """kmcpg_finalize_grouped: pairs uint32 [m, 2] (or PAIR_DTYPE [m]), read_offs uint64 [n + 2] as group_device wrote them."""
        p = params or default_params()
        pairs = np.ascontiguousarray(pairs)
        read_offs = np.ascontiguousarray(read_offs, dtype=np.uint64)
        qkmers = np.ascontiguousarray(qkmers, dtype=np.int32)
        qlen = np.ascontiguousarray(qlen, dtype=np.int32)
        assert pairs.dtype.itemsize in (4, 8) and len(read_offs) == len(qkmers) + 2
        r = Result()
        n = len(qkmers)
        _check(load().kmcpg_finalize_grouped(self._h, pairs.ctypes.data, read_offs.ctypes.data, qkmers.ctypes.data, qlen.ctypes.data, n, C.byref(p), C.byref(r)))
        if count_only:
            m = int(r.match_offs[n]) if n else 0
            load().kmcpg_result_free(C.byref(r))
            return m
        return _copy_result(r)

    def count_left_reads(self, pairs, read_offs, qkmers, qlen, params=None, left_refstats=None, left_cooccur=None, left_recount=None):
        """kmcpg_count_left_reads: the host half of the counting stages (K6, K7, K8) on a grouped list — pairs uint32 [m, 2] (or PAIR_DTYPE
        [m]), read_offs uint64 [n + 1] — into the handle's host state; left_*: a byte per read (non-zero = the stage takes it), None = every read."""
        p = params or default_params()
        pairs = np.ascontiguousarray(pairs)
        read_offs = np.ascontiguousarray(read_offs, dtype=np.uint64)
        qkmers = np.ascontiguousarray(qkmers, dtype=np.int32)
        qlen = np.ascontiguousarray(qlen, dtype=np.int32)
        n = len(qkmers)
        assert pairs.dtype.itemsize in (4, 8) and len(read_offs) == n + 1 and len(qlen) == n
        left = [None if l is None else np.ascontiguousarray(l, dtype=np.uint8) for l in (left_refstats, left_cooccur, left_recount)]
        assert all(l is None or len(l) == n for l in left)
        _check(load().kmcpg_count_left_reads(self._h, pairs.ctypes.data, read_offs.ctypes.data, qkmers.ctypes.data, qlen.ctypes.data, n, C.byref(p),
                                             *[None if l is None else l.ctypes.data for l in left]))

    # ---- statistics-only search: the counting stages and K10, no matches to the host ----------------------------
    def submit_stats(self, seqs, offs, seqs2=None, offs2=None, params=None):
        """kmcpg_submit_stats: submit's arguments on a handle with a counting stage on; the ticket is consumed by wait_stats only"""
        p = params or default_params()
        t = C.c_void_p()
        n = len(offs) - 1
        _check(load().kmcpg_submit_stats(self._h, seqs.ctypes.data, offs.ctypes.data, seqs2.ctypes.data if seqs2 is not None else None,
                                         offs2.ctypes.data if offs2 is not None else None, n, C.byref(p), C.byref(t)))
        return t

    def wait_stats(self, ticket):
        """kmcpg_wait_stats: dict of n_reads, matched_reads, kept_pairs, left_reads, left_pairs, bytes_d2h"""
        r = StatsResult()
        _check(load().kmcpg_wait_stats(ticket, C.byref(r)))
        return {f: int(getattr(r, f)) for f, _ in StatsResult._fields_}

    def search_stats(self, reads, reads2=None, params=None):
        """`reads` (list of bytes) through submit_stats / wait_stats: the counting stages' state on the handle is the result"""
        seqs, offs = pack_reads(reads)
        s2 = o2 = None
        if reads2 is not None:
            s2, o2 = pack_reads(reads2)
        return self.wait_stats(self.submit_stats(seqs, offs, s2, o2, params))

    def left_compact_device(self, d_pairs, d_read_offs, pair_cap, n, d_left_refstats, d_left_cooccur, d_left_recount, d_n_hits, hit_cap, d_mask,
                            d_left_pairs, left_cap, d_left_offs, stream=None):
        """kmcpg_left_compact_device on device pointers: the stages' LEFT bytes (None: the stage is not looked at) -> one mask byte per read,
        the pairs of the LEFT reads compacted behind d_left_pairs with their offsets (n + 1 words)."""
        _check(load().kmcpg_left_compact_device(self._h, d_pairs, d_read_offs, pair_cap, n, d_left_refstats, d_left_cooccur, d_left_recount, d_n_hits, hit_cap,
                                                d_mask, d_left_pairs, left_cap, d_left_offs, stream))

    def last_stats(self):
        """kmcpg_last_stats: (dict of the counters, [K4Launch] of the last K10 launch — empty below profiling level 1)"""
        st = StatsTicketStats()
        n = C.c_uint32(0)
        _check(load().kmcpg_last_stats(self._h, C.byref(st), None, 0, C.byref(n)))
        buf = (K4Launch * max(1, n.value))()
        _check(load().kmcpg_last_stats(self._h, C.byref(st), buf, n.value, C.byref(n)))
        self.last_k10_ms = float(st.k10_ms)  # HIP-event time of the stage's kernels (profiling level >= 1), else -1
        return {f: int(getattr(st, f)) for f, _ in StatsTicketStats._fields_ if f != "k10_ms"}, [buf[i] for i in range(n.value)]

    # ---- taxonomic binning: K11 behind K3 ----------------------------------------------------------------------
    def set_binning(self, node_of_column=None, parent=None, last=None, taxid=None):
        """kmcpg_set_binning: node_of_column one uint32 per global column (BIN_NO_NODE: not whitelisted); parent, last, taxid one uint32
        per node of the plan, numbered in pre-order with node 0 the virtual root; no argument = off."""
        if node_of_column is None:
            _check(load().kmcpg_set_binning(self._h, None, 0, None, None, None, 0))
            return
        c = np.ascontiguousarray(node_of_column, dtype=np.uint32)
        t = [np.ascontiguousarray(x, dtype=np.uint32) for x in (parent, last, taxid)]
        assert len(t[0]) == len(t[1]) == len(t[2])
        _check(load().kmcpg_set_binning(self._h, c.ctypes.data, len(c), t[0].ctypes.data, t[1].ctypes.data, t[2].ctypes.data, len(t[0])))

    def bin_device(self, d_pairs, d_read_offs, pair_cap, d_qkmers, n_reads, final_n, d_bins, d_n_hits=None, hit_cap=0, stream=None):
        """kmcpg_bin_device on device pointers: K3's pairs and offsets -> one uint32 per read (a TaxId, BIN_NONE or BIN_LEFT)."""
        _check(load().kmcpg_bin_device(self._h, d_pairs, d_read_offs, pair_cap, d_qkmers, n_reads, final_n, d_n_hits, hit_cap, d_bins, stream))

    def submit_bins(self, seqs, offs, seqs2=None, offs2=None, params=None):
        """kmcpg_submit_bins: submit's arguments on a handle with the binning stage on; the ticket is consumed by wait_bins only"""
        p = params or default_params()
        t = BinTicket()
        n = len(offs) - 1
        _check(load().kmcpg_submit_bins(self._h, seqs.ctypes.data, offs.ctypes.data, seqs2.ctypes.data if seqs2 is not None else None,
                                        offs2.ctypes.data if offs2 is not None else None, n, C.byref(p), C.byref(t)))
        t.n_reads = n
        return t

    def wait_bins(self, ticket):
        """kmcpg_wait_bins: (uint32 [n]: a TaxId or BIN_NONE per read, dict of n_reads, binned_reads, kept_pairs, host_reads, left_pairs,
        bytes_d2h, reruns).  A refused ticket stays valid and can be waited for again."""
        n = ticket.n_reads if isinstance(ticket, BinTicket) else 0  # (a ticket of another submit is refused before a word is written)
        bins = np.full(max(n, 1), BIN_LEFT, dtype=np.uint32)
        r = BinsResult()
        _check(load().kmcpg_wait_bins(ticket, bins.ctypes.data, C.byref(r)))
        return bins[:n], {f: int(getattr(r, f)) for f, _ in BinsResult._fields_}

    def search_bins(self, reads, reads2=None, params=None):
        """`reads` (list of bytes) through submit_bins / wait_bins"""
        seqs, offs = pack_reads(reads)
        s2 = o2 = None
        if reads2 is not None:
            s2, o2 = pack_reads(reads2)
        return self.wait_bins(self.submit_bins(seqs, offs, s2, o2, params))

    def last_bins(self):
        """kmcpg_last_bins: (dict of the counters, [K4Launch] of the last K11 launch — empty below profiling level 1)"""
        st = BinStats()
        n = C.c_uint32(0)
        _check(load().kmcpg_last_bins(self._h, C.byref(st), None, 0, C.byref(n)))
        buf = (K4Launch * max(1, n.value))()
        _check(load().kmcpg_last_bins(self._h, C.byref(st), buf, n.value, C.byref(n)))
        self.last_k11_ms = float(st.k11_ms)  # HIP-event time of the kernel (profiling level >= 1), else -1
        return {f: int(getattr(st, f)) for f, _ in BinStats._fields_ if f != "k11_ms"}, [buf[i] for i in range(n.value)]

    # ---- bench / parity support -----------------------------------------------------------------------
    def read_row_range(self, block, first_row, out):
        """rows first_row .. first_row+len(out)-1 of a resident block into `out` (uint8 [n, NumRowBytes], C-contiguous)."""
        assert out.flags["C_CONTIGUOUS"] and out.dtype == np.uint8
        _check(load().kmcpg_read_row_range(self._h, block, first_row, out.shape[0], out.ctypes.data))

    def plant(self, col, hashes):
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        _check(load().kmcpg_plant(self._h, col, hashes.ctypes.data, len(hashes)))

    def plant_reads_device(self, d_seqs, d_offs, n_reads, total_bases, max_read_len, d_cols, stream=None):
        _check(load().kmcpg_plant_reads_device(self._h, d_seqs, d_offs, n_reads, total_bases, max_read_len, d_cols, stream))

    def set_profiling(self, on=True):
        """False/0 off, True/1 kernel timing, 2 timing + count the row loads of the COBS kernel."""
        _check(load().kmcpg_set_profiling(self._h, int(on)))

    def last_gathered_bytes(self):
        n = C.c_uint64()
        _check(load().kmcpg_last_gathered_bytes(self._h, C.byref(n)))
        return n.value

    def last_tail_waves(self):
        """Waves of the last query_device call's COBS kernels that finished in tail mode (profiling level 2)."""
        n = C.c_uint64()
        _check(load().kmcpg_last_tail_waves(self._h, C.byref(n)))
        return n.value

    def _k2_launch_records(self):
        n = C.c_uint32(0)
        _check(load().kmcpg_last_k2_launches(self._h, None, 0, C.byref(n)))
        buf = (K2Launch * max(1, n.value))()
        _check(load().kmcpg_last_k2_launches(self._h, buf, n.value, C.byref(n)))
        return buf[:n.value]

    def last_k2_launches(self):
        """The COBS kernels the last query_device call launched, in launch order (profiling level >= 1): tuples
        (kind, lpr, lprb, npl, multi, group_rows, workgroups) with kind in K2_KINDS; lprb is 0 unless kind == "pair"."""
        return [(K2_KINDS[r.kind], r.lpr, r.lprb, r.npl, bool(r.multi), r.group_rows, r.workgroups) for r in self._k2_launch_records()]

    def last_k2_grids(self):
        """The workgroups each of those kernels was launched on, in the same order: equal to a record's `workgroups` except for the
        persistent short-read kernel (k2_cobs_persist), whose grid is what the chip holds at once or KMCPG_K2_PERSIST_WGS."""
        return [r.grid for r in self._k2_launch_records()]

    def last_hash_bytes(self):
        """Bytes of k-mer hashes the COBS kernel(s) of the last query_device call read (profiling level 2)."""
        n = C.c_uint64()
        _check(load().kmcpg_last_hash_bytes(self._h, C.byref(n)))
        return n.value

    def last_timing(self, age=0):
        """(k-mer kernels ms, COBS kernel ms) of the last query_device call (age 1: the one before, ... up to 3)."""
        a, b = C.c_float(), C.c_float()
        _check(load().kmcpg_timing_at(self._h, age, C.byref(a), C.byref(b)))
        return a.value, b.value

    def read_rows(self, block, row_idx):
        row_idx = np.ascontiguousarray(row_idx, dtype=np.uint64)
        rb = self.block_info(block)["row_bytes"]
        out = np.zeros((len(row_idx), rb), dtype=np.uint8)
        _check(load().kmcpg_read_rows(self._h, block, row_idx.ctypes.data, len(row_idx), out.ctypes.data))
        return out
