"""ABI of the statistics-only entry points (include/kmcp_gpu.h kmcpg_result_stats, kmcpg_stats_ticket_stats, KMCPG_K10_*): the ctypes
mirrors in kmcp_amd/lib.py have the C layout, as a C compiler lays the structs out from the header; the four entries are exported; and what
they refuse without a GPU, on a metadata-only handle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "shim", "testdata", "db", "R001")
EINVAL, EDEVICE = -1, -4
RESULT = ("n_reads", "matched_reads", "kept_pairs", "left_reads", "left_pairs", "bytes_d2h")
TICKET = RESULT + ("bad_segments", "skipped", "k10_ms")


def offsets(t, fields):
    return "printf(\"%zu" + " %zu" * len(fields) + "\\n\", sizeof(" + t + "), " + ", ".join(f"offsetof({t}, {f})" for f in fields) + ");\n"


SRC = ("#include <stddef.h>\n#include <stdio.h>\n#include \"kmcp_gpu.h\"\nint main(void) {\n" + offsets("kmcpg_result_stats", RESULT) + offsets("kmcpg_stats_ticket_stats", TICKET) +
       "printf(\"%d %d %d\\n\", KMCPG_K10_MASK, KMCPG_K10_COMPACT, KMCPG_K10_OFFS);\nreturn 0;\n}\n")


def test_layouts(tmp_path):
    from kmcp_amd import lib
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    (tmp_path / "w.c").write_text(SRC)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "w"), str(tmp_path / "w.c")], check=True)
    lines = subprocess.run([str(tmp_path / "w")], capture_output=True, text=True, check=True).stdout.splitlines()
    got = [[int(x) for x in l.split()] for l in lines]
    R, T = lib.StatsResult, lib.StatsTicketStats
    assert [f for f, _ in R._fields_] == list(RESULT) and [f for f, _ in T._fields_] == list(TICKET)
    assert got[0] == [C.sizeof(R)] + [getattr(R, f).offset for f in RESULT] == [48] + list(range(0, 48, 8))
    assert got[1] == [C.sizeof(T)] + [getattr(T, f).offset for f in TICKET] == [72] + list(range(0, 72, 8))
    assert got[2] == [lib.K10_MASK, lib.K10_COMPACT, lib.K10_OFFS] == [67, 68, 69]


def test_the_entries_are_exported():
    from kmcp_amd import lib
    L = lib.load()
    for sym in ("kmcpg_left_compact_device", "kmcpg_submit_stats", "kmcpg_wait_stats", "kmcpg_last_stats"):
        assert sym in lib.EXPORTS and getattr(L, sym)


def refused(fn, code):
    from kmcp_amd import lib
    with pytest.raises(lib.KmcpGpuError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def test_refusals_on_a_metadata_only_handle():
    from kmcp_amd import Database, lib
    seqs, offs = lib.pack_reads([b"ACGT" * 40, b"TTGCA" * 30])
    with Database.open(DB, device=-1) as db:
        n = int(db.info.n_cols)
        t = np.arange(n, dtype=np.uint32) // 2
        # no counting stage on: nothing to count, whatever the handle
        assert "no counting stage" in refused(lambda: db.submit_stats(seqs, offs), EINVAL)
        assert "together" in refused(lambda: db.submit_stats(seqs, offs, seqs, None), EINVAL)
        st, launches = db.last_stats()
        assert not any(st.values()) and launches == [] and db.last_k10_ms == -1
        # the species-specific stage beside a counting stage: K4 filters an output this ticket does not have
        db.set_refstats(t, None)
        db.set_specific(t, None)
        assert "kmcpg_set_specific" in refused(lambda: db.submit_stats(seqs, offs), EINVAL)
        db.set_specific()
        # a stage on, no GPU: the submit family's refusal
        assert "metadata-only" in refused(lambda: db.submit_stats(seqs, offs), EDEVICE)
        # the stage alone: argument checks first, then the device
        assert "left_cap" in refused(lambda: db.left_compact_device(8, 8, 4, 1, None, None, None, None, 0, 8, 8, 3, 8), EINVAL)
        assert "null" in refused(lambda: db.left_compact_device(8, None, 4, 1, None, None, None, None, 0, 8, 8, 4, 8), EINVAL)
        assert "metadata-only" in refused(lambda: db.left_compact_device(8, 8, 4, 1, None, None, None, None, 0, 8, 8, 4, 8), EDEVICE)
        db.set_refstats()
    # The wrong wait on a foreign ticket cannot be shown here: every submit entry needs a device (above), so no ticket of either kind can
    # exist without a GPU — tests/test_gpu_stats_only.py test_ticket_refusals holds the three waits against each other.  What is left
    # without one is no ticket at all: refused, nothing to give back
    r = lib.StatsResult()
    assert lib.load().kmcpg_wait_stats(None, C.byref(r)) == EINVAL
