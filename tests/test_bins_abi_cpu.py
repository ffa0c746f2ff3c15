"""ABI of the binning entry points (include/kmcp_gpu.h kmcpg_bin_stats, kmcpg_result_bins, KMCPG_K11_BIN, KMCPG_BIN_*): the ctypes mirrors
in kmcp_amd/lib.py have the C layout, as a C compiler lays the structs out from the header; the entries are exported; and what they refuse
without a GPU, on a metadata-only handle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "shim", "testdata", "db", "R001")
EINVAL, EDEVICE = -1, -4
STATS = ("no_bin", "one", "several", "left", "climb_steps", "bad_segments", "skipped", "grid", "in_lds", "k11_ms")
RESULT = ("n_reads", "binned_reads", "kept_pairs", "host_reads", "left_pairs", "bytes_d2h", "reruns")


def offsets(t, fields):
    return "printf(\"%zu" + " %zu" * len(fields) + "\\n\", sizeof(" + t + "), " + ", ".join(f"offsetof({t}, {f})" for f in fields) + ");\n"


SRC = ("#include <stddef.h>\n#include <stdio.h>\n#include \"kmcp_gpu.h\"\nint main(void) {\n" + offsets("kmcpg_bin_stats", STATS) + offsets("kmcpg_result_bins", RESULT) +
       "printf(\"%d %u %u %u\\n\", KMCPG_K11_BIN, KMCPG_BIN_NO_NODE, KMCPG_BIN_NONE, KMCPG_BIN_LEFT);\nreturn 0;\n}\n")


def test_layouts(tmp_path):
    from kmcp_amd import lib
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    (tmp_path / "w.c").write_text(SRC)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "w"), str(tmp_path / "w.c")], check=True)
    lines = subprocess.run([str(tmp_path / "w")], capture_output=True, text=True, check=True).stdout.splitlines()
    got = [[int(x) for x in l.split()] for l in lines]
    S, R = lib.BinStats, lib.BinsResult
    assert [f for f, _ in S._fields_] == list(STATS) and [f for f, _ in R._fields_] == list(RESULT)
    assert got[0] == [C.sizeof(S)] + [getattr(S, f).offset for f in STATS] == [72] + list(range(0, 56, 8)) + [56, 60, 64]
    assert got[1] == [C.sizeof(R)] + [getattr(R, f).offset for f in RESULT] == [56] + list(range(0, 56, 8))
    assert got[2] == [lib.K11_BIN, lib.BIN_NO_NODE, lib.BIN_NONE, lib.BIN_LEFT] == [70, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE]


def test_the_entries_are_exported():
    from kmcp_amd import lib
    L = lib.load()
    for sym in ("kmcpg_set_binning", "kmcpg_bin_device", "kmcpg_last_bins", "kmcpg_submit_bins", "kmcpg_wait_bins"):
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
        # the smallest plan: the virtual root and one node every column names
        cols = np.ones(n, dtype=np.uint32)
        parent, last, taxid = [0, 0], [1, 1], [0, 562]
        # the stage off: nothing to bin with, whatever the handle
        assert "kmcpg_set_binning" in refused(lambda: db.submit_bins(seqs, offs), EINVAL)
        assert "together" in refused(lambda: db.submit_bins(seqs, offs, seqs, None), EINVAL)
        st, launches = db.last_bins()
        assert not any(st.values()) and launches == [] and db.last_k11_ms == -1
        # what the plan must be: a pre-order numbering under node 0, columns that name its nodes or none, the handle's columns
        assert "node 0" in refused(lambda: db.set_binning(cols, [1, 0], last, taxid), EINVAL)
        assert "node 0" in refused(lambda: db.set_binning(cols, parent, [0, 1], taxid), EINVAL)
        assert "pre-order" in refused(lambda: db.set_binning(cols, [0, 1], last, taxid), EINVAL)
        assert "pre-order" in refused(lambda: db.set_binning(cols, parent, [1, 0], taxid), EINVAL)
        assert "pre-order" in refused(lambda: db.set_binning(np.zeros(n, dtype=np.uint32), [0, 0, 1], [2, 1, 2], [0, 5, 6]), EINVAL)  # last[2] > last[parent]
        assert "node_of_column[0]" in refused(lambda: db.set_binning(np.full(n, 2, dtype=np.uint32), parent, last, taxid), EINVAL)
        assert "sentinels" in refused(lambda: db.set_binning(cols, parent, last, [0, lib.BIN_LEFT]), EINVAL)
        assert "sentinels" in refused(lambda: db.set_binning(cols, parent, last, [0, lib.BIN_NONE]), EINVAL)
        assert "n_cols" in refused(lambda: db.set_binning(cols[:-1], parent, last, taxid), EINVAL)
        assert "virtual root" in refused(lambda: db.set_binning(cols, [], [], []), EINVAL)
        # a column off the whitelist is fine; the plan is kept without a GPU (the host half uses it)
        cols[0] = lib.BIN_NO_NODE
        db.set_binning(cols, parent, last, taxid)
        # the species-specific stage beside it: K4 filters an output this ticket does not have
        db.set_specific(np.arange(n, dtype=np.uint32) // 2, None)
        assert "kmcpg_set_specific" in refused(lambda: db.submit_bins(seqs, offs), EINVAL)
        db.set_specific()
        # the stage on, no GPU: the submit family's refusal; the stage alone: argument checks first, then the device
        assert "metadata-only" in refused(lambda: db.submit_bins(seqs, offs), EDEVICE)
        assert "null" in refused(lambda: db.bin_device(8, None, 4, 8, 1, 10, 8), EINVAL)
        assert "null" in refused(lambda: db.bin_device(8, 8, 4, 8, 1, 10, None), EINVAL)
        assert "metadata-only" in refused(lambda: db.bin_device(8, 8, 4, 8, 1, 10, 8), EDEVICE)
        db.set_binning()
        assert "kmcpg_set_binning" in refused(lambda: db.submit_bins(seqs, offs), EINVAL)
    # No ticket of any kind can exist without a GPU (every submit entry needs a device), so the waits are held against each other in
    # tests/test_gpu_binning.py.  What is left without one is no ticket at all: refused, nothing to give back
    r = lib.BinsResult()
    assert lib.load().kmcpg_wait_bins(None, None, C.byref(r)) == EINVAL
