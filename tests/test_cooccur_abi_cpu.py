"""ABI of the entry points of the shared reads of reference pairs (include/kmcp_gpu.h kmcpg_cooccur_pair, kmcpg_cooccur_totals,
kmcpg_cooccur_stats): the ctypes mirrors in kmcp_amd/lib.py have the C layout; on a metadata-only handle (no GPU) the stage goes on and
off, reads back an empty table, and refuses what it must; `kmcp-search --ref-stats-cooccur` refuses what it must before a file is opened
or a GPU touched — status 255 and the flag named; the dispatcher's spelling reaches kmcp-refstats."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "shim", "testdata", "db", "R001")
CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")
EINVAL, EDEVICE, EUNSUPPORTED = -1, -4, -6

SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "kmcp_gpu.h"
#define O(t, f) offsetof(t, f)
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(kmcpg_cooccur_pair), O(kmcpg_cooccur_pair, class_a), O(kmcpg_cooccur_pair, class_b), O(kmcpg_cooccur_pair, reads));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(kmcpg_cooccur_totals), O(kmcpg_cooccur_totals, multi_reads), O(kmcpg_cooccur_totals, device_adds),
         O(kmcpg_cooccur_totals, host_adds), O(kmcpg_cooccur_totals, left_full), O(kmcpg_cooccur_totals, host_reads), O(kmcpg_cooccur_totals, skipped_launches),
         O(kmcpg_cooccur_totals, table_slots), O(kmcpg_cooccur_totals, keys), O(kmcpg_cooccur_totals, rebuilds));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(kmcpg_cooccur_stats), O(kmcpg_cooccur_stats, empty), O(kmcpg_cooccur_stats, single),
         O(kmcpg_cooccur_stats, wave), O(kmcpg_cooccur_stats, left), O(kmcpg_cooccur_stats, left_full), O(kmcpg_cooccur_stats, pairs), O(kmcpg_cooccur_stats, lds_adds),
         O(kmcpg_cooccur_stats, global_adds), O(kmcpg_cooccur_stats, spilled_adds), O(kmcpg_cooccur_stats, claimed), O(kmcpg_cooccur_stats, skipped),
         O(kmcpg_cooccur_stats, bad_segments), O(kmcpg_cooccur_stats, grid), O(kmcpg_cooccur_stats, slots), O(kmcpg_cooccur_stats, k7_ms));
  printf("%d\n", KMCPG_K7_COOCCUR);
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
    d = lib.COOCCUR_DTYPE
    assert got[0] == [d.itemsize] + [d.fields[f][1] for f in ("class_a", "class_b", "reads")] == [16, 0, 4, 8]
    T, S = lib.CooccurTotals, lib.CooccurStats
    assert got[1] == [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_] == [72] + list(range(0, 72, 8))
    assert got[2] == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_] == [112] + list(range(0, 96, 8)) + [96, 100, 104]
    assert got[3] == [lib.K7_COOCCUR]


def test_the_entries_are_exported():
    from kmcp_amd import lib
    L = lib.load()
    for sym in ("kmcpg_set_cooccur", "kmcpg_cooccur_device", "kmcpg_cooccur_read", "kmcpg_cooccur_reset", "kmcpg_last_cooccur"):
        assert sym in lib.EXPORTS and getattr(L, sym)


def refused(fn, code):
    from kmcp_amd import lib
    with pytest.raises(lib.KmcpGpuError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def test_stage_on_and_off_on_a_metadata_only_handle(monkeypatch):
    from kmcp_amd import Database, default_params
    monkeypatch.delenv("KMCPG_COOCCUR_SLOTS", raising=False)
    with Database.open(DB, device=-1) as db:
        n = int(db.info.n_cols)
        t = np.arange(n, dtype=np.uint32) // 2
        empty = dict(multi_reads=0, device_adds=0, host_adds=0, left_full=0, host_reads=0, skipped_launches=0, keys=0, rebuilds=0)
        # off: nothing to read, to reset or to run
        refused(db.cooccur_read, EINVAL)
        refused(db.cooccur_reset, EINVAL)
        st, launches = db.last_cooccur()
        assert not any(st.values()) and launches == [] and db.last_k7_ms == -1
        # a bad table, bad sizes
        refused(lambda: db.set_cooccur(t[:-1]), EINVAL)
        assert "power of two" in refused(lambda: db.set_cooccur(t, table_slots=12), EINVAL)
        assert "power of two" in refused(lambda: db.set_cooccur(t, table_slots=1 << 31), EINVAL)
        for bad in ("3", "8192", "-2", "x"):
            monkeypatch.setenv("KMCPG_COOCCUR_SLOTS", bad)
            assert "KMCPG_COOCCUR_SLOTS" in refused(lambda: db.set_cooccur(t), EINVAL)
        refused(db.cooccur_read, EINVAL)  # still off
        # on, with the default table and with one of 8 slots, with and without the LDS table
        for slots, lds in ((0, None), (8, "0"), (1 << 20, "4096")):
            if lds is None:
                monkeypatch.delenv("KMCPG_COOCCUR_SLOTS")
            else:
                monkeypatch.setenv("KMCPG_COOCCUR_SLOTS", lds)
            db.set_cooccur(t, table_slots=slots)
            pairs, tot = db.cooccur_read()
            assert pairs.shape == (0,) and tot == dict(empty, table_slots=slots or 1 << 21)
            db.cooccur_reset()
            refused(lambda: db.cooccur_device(0, 0, 0, 0, 0, 512, 0), EINVAL)  # null offsets
            # what the stage refuses while it is on: the params K6 refuses, and every window submit
            seqs, offs = np.frombuffer(b"ACGT" * 40, dtype=np.uint8).copy(), np.array([0, 160], dtype=np.uint64)
            assert "try_se" in refused(lambda: db.search([b"ACGT" * 40], params=default_params(try_se=1)), EUNSUPPORTED)
            assert "top_n_scores" in refused(lambda: db.search([b"ACGT" * 40], params=default_params(top_n_scores=2)), EUNSUPPORTED)
            assert "kmcpg_set_cooccur" in refused(lambda: db.submit_windows(seqs, offs, 50, 100), EUNSUPPORTED)
        # independent of the two other stages behind K3
        s = (t // 2 + 1).astype(np.uint32)
        db.set_specific(t, s)
        db.set_refstats(t, s)
        db.cooccur_read()  # still on
        db.set_specific()
        db.set_refstats()
        db.cooccur_read()
        db.set_cooccur()
        refused(db.cooccur_read, EINVAL)
        db.set_refstats(t, s)
        db.refstats_read(n)  # ... and switching this stage off leaves that one on
        db.set_refstats()
        # off again: the params pass the stage's test (and fail later, for want of a GPU)
        refused(lambda: db.search([b"ACGT" * 40], params=default_params(try_se=1)), EDEVICE)


# ---- kmcp-search: none of these runs gets as far as a database (the -d directory and the input do not exist)
def search(tmp_path, args):
    if not os.path.exists(CLI):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # a GPU, were it asked for, would not be there
    return subprocess.run([CLI, "-d", str(tmp_path / "no-such-db"), str(tmp_path / "no-such-reads.fq"), "-o", str(tmp_path / "out.tsv")] + [str(a) for a in args],
                          capture_output=True, text=True, timeout=60, env=env)


def search_refused(tmp_path, args, *words):
    r = search(tmp_path, args)
    assert r.returncode == 255, (r.returncode, r.stderr)
    last = r.stderr.strip().splitlines()[-1]
    for w in words:
        assert w in last, (w, r.stderr)
    assert "no-such" not in r.stderr, r.stderr  # neither the database nor the input was looked at
    assert r.stdout == "" and not [f for f in ("out.tsv", "stats.tsv", "pairs.tsv") if (tmp_path / f).exists()]


def test_kmcp_search_refusals(tmp_path):
    stats, pairs, out = tmp_path / "stats.tsv", tmp_path / "pairs.tsv", tmp_path / "out.tsv"
    on = ["--ref-stats", stats, "--ref-stats-cooccur", pairs]
    # either new flag without --ref-stats
    search_refused(tmp_path, ["--ref-stats-cooccur", pairs], "--ref-stats-cooccur", "only used with --ref-stats")
    search_refused(tmp_path, ["--ref-stats-cooccur-slots", "1024"], "--ref-stats-cooccur-slots", "only used with --ref-stats")
    search_refused(tmp_path, ["--ref-stats", stats, "--ref-stats-cooccur-slots", "1024"], "--ref-stats-cooccur-slots", "only used with --ref-stats-cooccur")
    # the pairs do not go where the result or the statistics go
    search_refused(tmp_path, ["--ref-stats", stats, "--ref-stats-cooccur", out], "--ref-stats-cooccur", "must not be the search result's file")
    search_refused(tmp_path, ["--ref-stats", stats, "--ref-stats-cooccur", stats], "--ref-stats-cooccur", "must not be the statistics file")
    # a slot count that is not a power of two
    for bad in ("12", "-8", "3000000000"):
        search_refused(tmp_path, on + ["--ref-stats-cooccur-slots", bad], "--ref-stats-cooccur-slots", "power of two")
    search_refused(tmp_path, on + ["--ref-stats-cooccur-slots", "x"], "invalid argument", "ref-stats-cooccur-slots")
    # everything --ref-stats refuses
    for extra, word in ((["-K"], "-K/--keep-unmatched"), (["--try-se"], "--try-se"), (["-n", "2"], "-n/--keep-top-scores"),
                        (["--sliding-step", "100", "--sliding-window", "300"], "--sliding-"), (["--gpus", "2"], "--gpus/--gpu-ids"), (["--gpu-passes", "2"], "--gpu-passes")):
        search_refused(tmp_path, on + extra, word, "--ref-stats")
    search_refused(tmp_path, on + ["--ref-stats-mode", "0"], "--ref-stats-mode 0", "kmcp-refstats")


@pytest.mark.parametrize("extra", [[], ["--ref-stats-cooccur-slots", "0"], ["--ref-stats-cooccur-slots", "65536", "--ref-stats-level", "strain"]], ids=["plain", "default slots", "slots"])
def test_the_accepted_forms_get_as_far_as_the_input(tmp_path, extra):
    r = search(tmp_path, ["--ref-stats", tmp_path / "stats.tsv", "--ref-stats-cooccur", tmp_path / "pairs.tsv"] + extra)
    assert r.returncode == 255 and "no-such-reads.fq" in r.stderr and not (tmp_path / "out.tsv").exists() and not (tmp_path / "pairs.tsv").exists()


def test_the_dispatcher_spelling(tmp_path):
    from tests import cooccur_reference as CR
    from tests import filter_cases as FC
    rows = [FC.row("u1", "a1"), FC.row("u2", "b1"), FC.row("q", "a1"), FC.row("q", "b1")]
    f, out = tmp_path / "in.tsv", tmp_path / "pairs.tsv"
    f.write_text("".join(rows))
    r = subprocess.run([os.path.join(ROOT, "kmcp_amd", "kmcp"), "-q", "utils", "ref-stats", "--level", "strain", "--cooccur", str(out), str(f)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert out.read_text() == CR.cooccur(["".join(rows)], level="strain") == "# pairs: 1\n#refA\trefB\treads\na1\tb1\t1\n"
    help_text = subprocess.run([os.path.join(ROOT, "kmcp_amd", "kmcp"), "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--cooccur" in help_text
