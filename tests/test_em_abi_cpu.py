"""ABI of the entry points of an EM pass (include/kmcp_gpu.h kmcpg_em_class, kmcpg_em_col, kmcpg_em_totals, kmcpg_em_stats): the ctypes
mirrors and dtypes in kmcp_amd/lib.py have the C layout; on a metadata-only handle (no GPU) a pass runs over the empty logs of the recount
stage and refuses what it must."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "shim", "testdata", "db", "R001")
EINVAL = -1

COL = ("match", "uniq", "hic", "single_bases", "bases_lo", "bases_hi")
TOTALS = ("assigned_reads", "unique_reads", "split_reads", "host_reads")
STATS = ("reads", "none", "one", "split", "lds_adds", "global_adds", "spilled_adds", "grid", "slots", "em_ms")


def offsets(t, fields):
    return "printf(\"%zu" + " %zu" * len(fields) + "\\n\", sizeof(" + t + "), " + ", ".join(f"offsetof({t}, {f})" for f in fields) + ");\n"


SRC = ("#include <stddef.h>\n#include <stdio.h>\n#include \"kmcp_gpu.h\"\nint main(void) {\n" + offsets("kmcpg_em_class", ("est", "reserved", "coverage")) +
       offsets("kmcpg_em_col", COL) + offsets("kmcpg_em_totals", TOTALS) + offsets("kmcpg_em_stats", STATS) + "printf(\"%d\\n\", KMCPG_K9_EM);\nreturn 0;\n}\n")


def test_layouts(tmp_path):
    from kmcp_amd import lib
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    (tmp_path / "w.c").write_text(SRC)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "w"), str(tmp_path / "w.c")], check=True)
    lines = subprocess.run([str(tmp_path / "w")], capture_output=True, text=True, check=True).stdout.splitlines()
    got = [[int(x) for x in l.split()] for l in lines]
    d = lib.EM_CLASS_DTYPE
    assert got[0] == [d.itemsize] + [d.fields[f][1] for f in ("est", "reserved", "coverage")] == [16, 0, 4, 8]
    d = lib.EM_COL_DTYPE
    assert d.names == COL and got[1] == [d.itemsize] + [d.fields[f][1] for f in COL] == [48] + list(range(0, 48, 8))
    T, S = lib.EmTotals, lib.EmStats
    assert [f for f, _ in T._fields_] == list(TOTALS) and [f for f, _ in S._fields_] == list(STATS)
    assert got[2] == [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_] == [32, 0, 8, 16, 24]
    assert got[3] == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_] == [72] + list(range(0, 56, 8)) + [56, 60, 64]
    assert got[4] == [lib.K9_EM] == [66]
    assert lib.EM_UNIT == 720720 << 12 == 2952069120 < 1 << 32


def test_the_entries_are_exported():
    from kmcp_amd import lib
    L = lib.load()
    for sym in ("kmcpg_em_pass", "kmcpg_em_read", "kmcpg_last_em"):
        assert sym in lib.EXPORTS and getattr(L, sym)


def refused(fn, code):
    from kmcp_amd import lib
    with pytest.raises(lib.KmcpGpuError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def test_a_pass_on_a_metadata_only_handle(monkeypatch):
    from kmcp_amd import Database, lib
    monkeypatch.delenv("KMCPG_EM_SLOTS", raising=False)
    with Database.open(DB, device=-1) as db:
        n = int(db.info.n_cols)
        t = np.arange(n, dtype=np.uint32) // 2
        s = (t // 2 + 1).astype(np.uint32)
        classes = np.zeros(int(t.max()) + 1, dtype=lib.EM_CLASS_DTYPE)
        classes["est"], classes["coverage"] = 1, 2.5
        # the recount stage off: nothing to pass over, nothing to read
        assert "stage is off" in refused(lambda: db.em_pass(classes), EINVAL)
        assert "stage is off" in refused(db.em_read, EINVAL)
        st, launches = db.last_em()
        assert not any(st.values()) and launches == [] and db.last_k9_ms == -1
        db.set_recount(t, s)
        assert "kmcpg_em_pass first" in refused(db.em_read, EINVAL)
        # an estimated class needs a finite coverage above 0; a class outside the whitelist needs none
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            c = classes.copy()
            c["coverage"][1] = bad
            assert "coverage" in refused(lambda: db.em_pass(c), EINVAL)
            c["est"][1] = 0
            db.em_pass(c)
        for bad in ("3", "2048", "-2", "x"):
            monkeypatch.setenv("KMCPG_EM_SLOTS", bad)
            assert "KMCPG_EM_SLOTS" in refused(lambda: db.em_pass(classes), EINVAL)
        for slots in ("0", "2", "1024"):
            monkeypatch.setenv("KMCPG_EM_SLOTS", slots)
            db.em_pass(classes, level_species=False)
        monkeypatch.delenv("KMCPG_EM_SLOTS")
        db.em_pass(classes)
        cols, tot = db.em_read()
        assert cols.shape == (n,) and cols.dtype == lib.EM_COL_DTYPE and not cols.view(np.uint64).any() and tot == {k: 0 for k in TOTALS}
        db.em_pass(classes[:0])  # no class at all: fine
        # the recount's own calls are what they are beside a pass
        rc = np.zeros(len(classes), dtype=lib.RECOUNT_CLASS_DTYPE)
        rc["kept"] = 1
        db.recount_run(rc, np.zeros(0, dtype=lib.COOCCUR_DTYPE))
        before = db.recount_read()
        db.em_pass(classes)
        after = db.recount_read()
        assert before[0].tobytes() == after[0].tobytes() and before[1] == after[1]
        # a reset or a new stage forgets the pass
        db.recount_reset()
        assert "kmcpg_em_pass first" in refused(db.em_read, EINVAL)
        db.em_pass(classes)
        db.set_recount(t, s)
        assert "kmcpg_em_pass first" in refused(db.em_read, EINVAL)
        db.set_recount()
        assert "stage is off" in refused(lambda: db.em_pass(classes), EINVAL)
