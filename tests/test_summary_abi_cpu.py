"""ABI of the window-summary entry points (include/kmcp_gpu.h kmcpg_window_summary, kmcpg_result_summaries, kmcpg_summary_stats): the ctypes
mirrors in kmcp_amd/lib.py have the C layout, as a C compiler lays the structs out from the header."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "kmcp_gpu.h"
#define O(t, f) offsetof(t, f)
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(kmcpg_window_summary), O(kmcpg_window_summary, n_targets), O(kmcpg_window_summary, flags), O(kmcpg_window_summary, score));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(kmcpg_result_summaries), O(kmcpg_result_summaries, n_windows), O(kmcpg_result_summaries, qlen),
         O(kmcpg_result_summaries, qkmers), O(kmcpg_result_summaries, s), O(kmcpg_result_summaries, owner));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(kmcpg_summary_stats), O(kmcpg_summary_stats, single), O(kmcpg_summary_stats, wave),
         O(kmcpg_summary_stats, left), O(kmcpg_summary_stats, empty), O(kmcpg_summary_stats, left_pairs), O(kmcpg_summary_stats, bytes_d2h),
         O(kmcpg_summary_stats, bad_segments), O(kmcpg_summary_stats, k5_ms));
  printf("%u %u %d %d\n", KMCPG_SUMMARY_LEFT, KMCPG_SUMMARY_HOST, KMCPG_K5_SUMMARY, KMCPG_K5_COMPACT);
  return 0;
}
'''


def test_summary_layouts(tmp_path):
    from kmcp_amd import lib
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    (tmp_path / "w.c").write_text(SRC)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "w"), str(tmp_path / "w.c")], check=True)
    lines = subprocess.run([str(tmp_path / "w")], capture_output=True, text=True, check=True).stdout.splitlines()
    got = [[int(x) for x in l.split()] for l in lines]
    W, R, S = lib.WindowSummary, lib.ResultSummaries, lib.SummaryStats
    assert got[0] == [C.sizeof(W), W.n_targets.offset, W.flags.offset, W.score.offset] == [16, 0, 4, 8]
    d = lib.SUMMARY_DTYPE
    assert [d.itemsize] + [d.fields[f][1] for f in ("n_targets", "flags", "score")] == got[0]
    assert d == np.dtype([("n_targets", "<u4"), ("flags", "<u4"), ("score", "<f8")])
    assert got[1] == [C.sizeof(R), R.n_windows.offset, R.qlen.offset, R.qkmers.offset, R.s.offset, R.owner.offset] == [40, 0, 8, 16, 24, 32]
    assert got[2] == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_] == [64, 0, 8, 16, 24, 32, 40, 48, 56]
    assert got[3] == [lib.SUMMARY_LEFT, lib.SUMMARY_HOST, lib.K5_SUMMARY, lib.K5_COMPACT]


def test_the_entries_are_exported():
    from kmcp_amd import lib
    L = lib.load()
    for sym in ("kmcpg_summarize_device", "kmcpg_last_summary", "kmcpg_submit_windows_summary", "kmcpg_wait_summaries", "kmcpg_result_summaries_free"):
        assert sym in lib.EXPORTS and getattr(L, sym)
