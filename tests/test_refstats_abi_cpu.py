"""ABI of the reference-statistics entry points (include/kmcp_gpu.h kmcpg_col_stats, kmcpg_refstats_totals, kmcpg_refstats_stats): the ctypes
mirrors in kmcp_amd/lib.py have the C layout; and on a metadata-only handle (no GPU) the stage goes on and off, reads back zeroed
counters, and refuses what it must."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "shim", "testdata", "db", "R001")
EINVAL, EDEVICE, EUNSUPPORTED = -1, -4, -6

SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "kmcp_gpu.h"
#define O(t, f) offsetof(t, f)
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(kmcpg_col_stats), O(kmcpg_col_stats, rows), O(kmcpg_col_stats, firsts), O(kmcpg_col_stats, ureads), O(kmcpg_col_stats, hic_ureads));
  printf("%zu %zu %zu %zu %zu\n", sizeof(kmcpg_refstats_totals), O(kmcpg_refstats_totals, matched_reads), O(kmcpg_refstats_totals, unique_reads),
         O(kmcpg_refstats_totals, host_reads), O(kmcpg_refstats_totals, skipped_launches));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(kmcpg_refstats_stats), O(kmcpg_refstats_stats, empty), O(kmcpg_refstats_stats, single),
         O(kmcpg_refstats_stats, wave), O(kmcpg_refstats_stats, left), O(kmcpg_refstats_stats, lds_adds), O(kmcpg_refstats_stats, global_adds),
         O(kmcpg_refstats_stats, spilled_adds), O(kmcpg_refstats_stats, skipped), O(kmcpg_refstats_stats, bad_segments), O(kmcpg_refstats_stats, grid),
         O(kmcpg_refstats_stats, slots), O(kmcpg_refstats_stats, k6_ms));
  printf("%d\n", KMCPG_K6_REFSTATS);
  return 0;
}
'''


def test_layouts(tmp_path):
    from kmcp_amd import lib
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    (tmp_path / "w.c").write_text(SRC)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "w"), str(tmp_path / "w.c")], check=True)
    lines = subprocess.run([str(tmp_path / "w")], capture_output=True, text=True, check=True).stdout.splitlines()
    got = [[int(x) for x in l.split()] for l in lines]
    d = lib.COL_STATS_DTYPE
    assert got[0] == [d.itemsize] + [d.fields[f][1] for f in ("rows", "firsts", "ureads", "hic_ureads")] == [32, 0, 8, 16, 24]
    T, S = lib.RefstatsTotals, lib.RefstatsStats
    assert got[1] == [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_] == [32, 0, 8, 16, 24]
    assert got[2] == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_] == [88, 0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80]
    assert got[3] == [lib.K6_REFSTATS]


def test_the_entries_are_exported():
    from kmcp_amd import lib
    L = lib.load()
    for sym in ("kmcpg_set_refstats", "kmcpg_refstats_device", "kmcpg_refstats_read", "kmcpg_refstats_reset", "kmcpg_last_refstats"):
        assert sym in lib.EXPORTS and getattr(L, sym)


def refused(fn, code):
    from kmcp_amd import lib
    with pytest.raises(lib.KmcpGpuError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def test_stage_on_and_off_on_a_metadata_only_handle():
    from kmcp_amd import Database, default_params
    with Database.open(DB, device=-1) as db:
        n = int(db.info.n_cols)
        t = np.arange(n, dtype=np.uint32) // 2
        s = (t // 2 + 1).astype(np.uint32)
        # off: nothing to read, to reset or to run
        refused(lambda: db.refstats_read(n), EINVAL)
        refused(db.refstats_reset, EINVAL)
        st, launches = db.last_refstats()
        assert not any(st.values()) and launches == [] and db.last_k6_ms == -1
        # bad tables
        refused(lambda: db.set_refstats(t[:-1], s[:-1]), EINVAL)
        refused(lambda: db.set_refstats(t, s, hic_min_qcov=1.5), EINVAL)
        refused(lambda: db.set_refstats(t, s, hic_min_qcov=-0.1), EINVAL)
        refused(lambda: db.set_refstats(t, s, hic_min_qcov=float("nan")), EINVAL)
        # on, at both levels; independent of the species-specific stage
        for species in (s, None):
            db.set_refstats(t, species, hic_min_qcov=0.75)
            cols, tot = db.refstats_read(n)
            assert cols.shape == (n,) and not cols.view(np.uint64).any() and tot == dict(matched_reads=0, unique_reads=0, host_reads=0, skipped_launches=0)
            refused(lambda: db.refstats_read(n - 1), EINVAL)
            db.refstats_reset()
            refused(lambda: db.refstats_device(0, 0, 0, 0, 0, 512, 0), EINVAL)  # null offsets
            # what the stage refuses while it is on: the params K4 refuses, and every window submit
            seqs, offs = np.frombuffer(b"ACGT" * 40, dtype=np.uint8).copy(), np.array([0, 160], dtype=np.uint64)
            assert "try_se" in refused(lambda: db.search([b"ACGT" * 40], params=default_params(try_se=1)), EUNSUPPORTED)
            assert "top_n_scores" in refused(lambda: db.search([b"ACGT" * 40], params=default_params(top_n_scores=2)), EUNSUPPORTED)
            assert "kmcpg_set_refstats" in refused(lambda: db.submit_windows(seqs, offs, 50, 100), EUNSUPPORTED)
        db.set_specific(t, s)
        cols, _ = db.refstats_read(n)  # still on
        db.set_specific()
        db.set_refstats()
        refused(lambda: db.refstats_read(n), EINVAL)
        # off again: the params pass the stage's test (and fail later, for want of a GPU)
        refused(lambda: db.search([b"ACGT" * 40], params=default_params(try_se=1)), EDEVICE)
