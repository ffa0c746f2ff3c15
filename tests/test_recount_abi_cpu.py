"""ABI of the entry points of the recount with ambiguity correction (include/kmcp_gpu.h kmcpg_recount_col, kmcpg_recount_class,
kmcpg_recount_params, kmcpg_recount_totals, kmcpg_recount_stats): the ctypes mirrors and dtypes in kmcp_amd/lib.py have the C layout; on
a metadata-only handle (no GPU) the stage goes on and off, replays its empty logs, and refuses what it must."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "shim", "testdata", "db", "R001")
EINVAL, EDEVICE, EUNSUPPORTED = -1, -4, -6

TOTALS = ("recounted_reads", "unique_reads", "corrected_reads", "single_reads", "replayed_reads", "host_reads", "left_full", "skipped_launches", "log_bytes",
          "log_bytes_used", "logged_reads")
STATS = ("empty", "single", "logged", "left", "left_full", "lds_adds", "global_adds", "spilled_adds", "skipped", "bad_segments", "log_bytes_used", "replay_reads",
         "replay_recounted", "replay_corrected", "replay_unique", "replay_lookups", "replay_lds_adds", "replay_global_adds", "replay_spilled_adds", "grid", "slots",
         "replay_grid", "reserved", "log_ms", "replay_ms")


def offsets(t, fields):
    return "printf(\"%zu" + " %zu" * len(fields) + "\\n\", sizeof(" + t + "), " + ", ".join(f"offsetof({t}, {f})" for f in fields) + ");\n"


SRC = ("#include <stddef.h>\n#include <stdio.h>\n#include \"kmcp_gpu.h\"\nint main(void) {\n" + offsets("kmcpg_recount_col", ("match", "uniq", "hic", "bases")) +
       offsets("kmcpg_recount_class", ("kept", "reserved", "reads", "ureads")) + offsets("kmcpg_recount_params", ("one_minus_d", "r_err", "no_amb_corr", "level_species")) +
       offsets("kmcpg_recount_totals", TOTALS) + offsets("kmcpg_recount_stats", STATS) + "printf(\"%d %d\\n\", KMCPG_K8_LOG, KMCPG_K8_REPLAY);\nreturn 0;\n}\n")


def test_layouts(tmp_path):
    from kmcp_amd import lib
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    (tmp_path / "w.c").write_text(SRC)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "w"), str(tmp_path / "w.c")], check=True)
    lines = subprocess.run([str(tmp_path / "w")], capture_output=True, text=True, check=True).stdout.splitlines()
    got = [[int(x) for x in l.split()] for l in lines]
    d = lib.RECOUNT_DTYPE
    assert got[0] == [d.itemsize] + [d.fields[f][1] for f in ("match", "uniq", "hic", "bases")] == [32, 0, 8, 16, 24]
    d = lib.RECOUNT_CLASS_DTYPE
    assert got[1] == [d.itemsize] + [d.fields[f][1] for f in ("kept", "reserved", "reads", "ureads")] == [24, 0, 4, 8, 16]
    P, T, S = lib.RecountParams, lib.RecountTotals, lib.RecountStats
    assert got[2] == [C.sizeof(P)] + [getattr(P, f).offset for f, _ in P._fields_] == [24, 0, 8, 16, 20]
    assert [f for f, _ in T._fields_] == list(TOTALS) and [f for f, _ in S._fields_] == list(STATS)
    assert got[3] == [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_] == [88] + list(range(0, 88, 8))
    assert got[4] == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_] == [184] + list(range(0, 152, 8)) + [152, 156, 160, 164, 168, 176]
    assert got[5] == [lib.K8_LOG, lib.K8_REPLAY] == [64, 65]
    assert (lib.RECOUNT_UNIT, lib.RECOUNT_BASE_UNIT) == (720720, 65536)


def test_the_entries_are_exported():
    from kmcp_amd import lib
    L = lib.load()
    for sym in ("kmcpg_set_recount", "kmcpg_recount_log_device", "kmcpg_recount_run", "kmcpg_recount_read", "kmcpg_recount_reset", "kmcpg_last_recount"):
        assert sym in lib.EXPORTS and getattr(L, sym)


def refused(fn, code):
    from kmcp_amd import lib
    with pytest.raises(lib.KmcpGpuError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def test_stage_on_and_off_on_a_metadata_only_handle(monkeypatch):
    from kmcp_amd import Database, default_params, lib
    monkeypatch.delenv("KMCPG_RECOUNT_SLOTS", raising=False)
    with Database.open(DB, device=-1) as db:
        n = int(db.info.n_cols)
        t = np.arange(n, dtype=np.uint32) // 2
        s = (t // 2 + 1).astype(np.uint32)
        classes = np.zeros(int(t.max()) + 1, dtype=lib.RECOUNT_CLASS_DTYPE)
        classes["kept"] = 1
        none = np.zeros(0, dtype=lib.COOCCUR_DTYPE)
        # off: nothing to run, to read or to reset
        refused(lambda: db.recount_run(classes, none), EINVAL)
        refused(db.recount_reset, EINVAL)
        st, launches = db.last_recount()
        assert not any(st.values()) and launches == [] and db.last_k8_log_ms == db.last_k8_replay_ms == -1
        # bad tables, bad sizes
        refused(lambda: db.set_recount(t[:-1], s[:-1]), EINVAL)
        for bad in (8, 63, (4 << 30) + 8):
            assert "log_bytes" in refused(lambda: db.set_recount(t, s, log_bytes=bad), EINVAL)
        for bad in ("3", "2048", "-2", "x"):
            monkeypatch.setenv("KMCPG_RECOUNT_SLOTS", bad)
            assert "KMCPG_RECOUNT_SLOTS" in refused(lambda: db.set_recount(t, s), EINVAL)
        refused(db.recount_reset, EINVAL)  # still off
        for log_bytes, lds, species in ((0, None, s), (64, "0", None), (1 << 20, "1024", s)):
            if lds is None:
                monkeypatch.delenv("KMCPG_RECOUNT_SLOTS")
            else:
                monkeypatch.setenv("KMCPG_RECOUNT_SLOTS", lds)
            db.set_recount(t, species, hic_min_qcov=0.75, log_bytes=log_bytes)
            assert "kmcpg_recount_run first" in refused(db.recount_read, EINVAL)
            db.recount_run(classes, none, no_amb_corr=True, level_species=False)
            cols, tot = db.recount_read()
            assert cols.shape == (n,) and not cols.view(np.uint64).any()
            assert tot == dict({k: 0 for k in TOTALS}, log_bytes=log_bytes or 256 << 20)
            # the pair list must be what kmcpg_cooccur_read returns
            assert "sorted" in refused(lambda: db.recount_run(classes, np.array([(2, 3, 1), (1, 2, 1)], dtype=lib.COOCCUR_DTYPE)), EINVAL)
            assert "sorted" in refused(lambda: db.recount_run(classes, np.array([(1, 2, 1), (1, 2, 1)], dtype=lib.COOCCUR_DTYPE)), EINVAL)
            assert "class_a" in refused(lambda: db.recount_run(classes, np.array([(2, 2, 1)], dtype=lib.COOCCUR_DTYPE)), EINVAL)
            db.recount_run(classes[:0], np.array([(1, 2, 5), (1, 3, 1)], dtype=lib.COOCCUR_DTYPE))  # no class is kept: fine
            db.recount_reset()
            assert "kmcpg_recount_run first" in refused(db.recount_read, EINVAL)
            refused(lambda: db.recount_log_device(0, 0, 0, 0, 0, 0, 512, 0), EINVAL)  # null offsets
            # what the stage refuses while it is on: the params K6 refuses, and every window submit
            seqs, offs = np.frombuffer(b"ACGT" * 40, dtype=np.uint8).copy(), np.array([0, 160], dtype=np.uint64)
            assert "try_se" in refused(lambda: db.search([b"ACGT" * 40], params=default_params(try_se=1)), EUNSUPPORTED)
            assert "top_n_scores" in refused(lambda: db.search([b"ACGT" * 40], params=default_params(top_n_scores=2)), EUNSUPPORTED)
            assert "kmcpg_set_recount" in refused(lambda: db.submit_windows(seqs, offs, 50, 100), EUNSUPPORTED)
        # independent of the other stages behind K3
        db.set_specific(t, s)
        db.set_refstats(t, s)
        db.set_cooccur(t)
        db.recount_run(classes, none)  # still on
        db.set_specific()
        db.set_refstats()
        db.set_cooccur()
        db.recount_run(classes, none)
        db.set_recount()
        refused(lambda: db.recount_run(classes, none), EINVAL)
        db.set_cooccur(t)
        db.cooccur_read()  # ... and switching this stage off leaves that one on
        db.set_cooccur()
        # off again: the params pass the stage's test (and fail later, for want of a GPU)
        refused(lambda: db.search([b"ACGT" * 40], params=default_params(try_se=1)), EDEVICE)
