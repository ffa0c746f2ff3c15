"""The host side of kmcp-makedb without a GPU: the chunk bounds of kmcp_amd/csrc/split_plan.hpp (`kmcp compute --split-number`,
compute.go:675-744) against tests/synth.py split_chunks plus the reference's drop rule, exhaustively over small sequences and for a
handful near 2^32 (tests/split_check.cpp); kmcpg_split_bounds through the binding; kmcp-makedb's flag parsing and refusals (exit
status 255 as checkError gives), and its record join and --seq-name-filter on a small FASTA (`--dry-run` prints what would be sketched)."""
import gzip
import os
import subprocess

import pytest

from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAKEDB = os.path.join(ROOT, "kmcp_amd", "kmcp-makedb")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from kmcp_amd import lib
    if not (os.path.exists(lib.LIB_PATH) and os.path.exists(MAKEDB)):
        g.build()
    return lib


def want_bounds(L, n, overlap, min_ref, k):
    """synth.split_chunks over range(L) — a sequence whose slices say where they start — then compute.go:713"""
    seq = range(L)
    chunks = [seq] if (n <= 1 or L < min_ref) else synth.split_chunks(seq, n, overlap)
    return [(c.start if len(c) else 0, (c.start if len(c) else 0) + len(c)) for c in chunks if not (len(c) - 1 <= overlap or len(c) < k)]


def cases():
    for L in range(0, 3001):
        for n in (1, 2, 3, 10, 17):
            for overlap in (0, 1, 150, 999):
                for min_ref in (0, 1000):
                    for k in (11, 21, 64):
                        yield L, n, overlap, min_ref, k
    for L in (2**32 - 1, 2**32, 2**32 + 1, 2**32 + 12345, 2**33 + 7, 2**32 - 999):
        for n in (1, 2, 10, 17, 65535):
            for overlap in (0, 150, 999):
                yield L, n, overlap, 0, 21
                yield L, n, overlap, 2**34, 21


def test_split_bounds_equal_synth_split_chunks(tmp_path):
    exe, path = str(tmp_path / "split_check"), str(tmp_path / "cases.txt")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "split_check.cpp")], check=True)
    total = 0
    with open(path, "w") as fh:
        for L, n, overlap, min_ref, k in cases():
            w = want_bounds(L, n, overlap, min_ref, k)
            fh.write("%d %d %d %d %d %d %s\n" % (L, n, overlap, min_ref, k, len(w), " ".join("%d %d" % b for b in w)))
            total += 1
    assert total == 3001 * 5 * 4 * 2 * 3 + 6 * 5 * 3 * 2
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("%d cases, 0 wrong" % total), r.stdout


def test_split_bounds_binding(built):
    lib = built
    assert lib.split_bounds(1000, 3, 10, 0, 21) == want_bounds(1000, 3, 10, 0, 21) == [(0, 340), (330, 670), (660, 1000)]
    assert lib.split_bounds(999, 10, 150, 1000, 21) == [(0, 999)]
    assert lib.split_bounds(20, 1, 0, 0, 21) == []
    assert lib.split_bounds(2**32 + 5, 10, 150, 0, 31) == want_bounds(2**32 + 5, 10, 150, 0, 31)
    with pytest.raises(lib.KmcpGpuError):
        lib.split_bounds(1000, 70000, 0, 0, 21)  # compute.go:295
    with pytest.raises(lib.KmcpGpuError):
        lib.split_bounds(1000, 2, 0, 0, 0)


def run(args):
    return subprocess.run([MAKEDB] + args, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args, word", [
    (["--circular"], "--circular"),
    (["--by-seq"], "--by-seq"),
    (["-s", "1000"], "--split-size"),
    (["--split-size", "1000"], "--split-size"),
    (["-W", "8", "-S", "11"], "--minimizer-w and --syncmer-s"),
    (["-k", "65"], "should be <=64"),
    (["-k", "0"], "invalid k"),
    (["-k", "21,31"], "-k/--kmer"),
    (["-n", "70000"], "--split-number"),
    (["--num-hash", "0"], "--num-hash"),
    (["-f", "1.5"], "--false-positive-rate"),
    (["--no-such-flag"], "--no-such-flag"),
])
def test_makedb_refuses(built, tmp_path, args, word):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGTACGT\n")
    base = ["-O", str(tmp_path / "out.kmcp"), str(fa)]
    if "-k" not in args:
        base = ["-k", "21"] + base
    r = run(args + base)
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert word in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out.kmcp")


def test_makedb_needs_k_out_dir_and_files(built, tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGT\n")
    for args, word in ((["-O", str(tmp_path / "o"), str(fa)], "flag -k/--kmer needed"),
                       (["-k", "21", str(fa)], "flag -O/--out-dir is needed"),
                       (["-k", "21", "-O", str(tmp_path / "o")], "FASTA/Q files needed")):
        r = run(args)
        assert r.returncode == 255 and word in r.stderr, (args, r.stderr)
    assert run(["--help"]).returncode == 0


def test_makedb_joins_records_and_filters_names(built, tmp_path):
    """--dry-run: one line per reference — name, joined length, chunks — and no GPU is touched"""
    recs = [("chr1 some chromosome", "ACGTTGCAAC" * 30), ("p1 plasmid pX", "GGGGGCCCCC" * 9), ("chr2", "TTGACCAGTA" * 20), ("p2 Plasmid", "AC" * 50)]
    fa = tmp_path / "GCF_000001.1_x.fa.gz"
    with gzip.open(fa, "wt") as fh:
        for n, s in recs:
            fh.write(">%s\n" % n)
            for i in range(0, len(s), 70):
                fh.write(s[i:i + 70] + "\n")
    only = tmp_path / "GCF_000002.2.fna"
    only.write_text(">q plasmid\nACGTACGTAGCTAGCTAGCATCGATCGATCAGCTACGACTAGC\n")
    lst = tmp_path / "list.txt"
    lst.write_text("%s\n%s\n" % (fa, only))
    k = 21
    r = run(["-k", str(k), "-n", "3", "-l", "10", "-m", "0", "-B", "plasmid", "-O", str(tmp_path / "o.kmcp"), "--dry-run", "-i", str(lst)])
    assert r.returncode == 0, r.stderr
    # p1 and p2 go (the reference prefixes (?i) to every -B expression, compute.go:251): chr1 + N*20 + chr2
    L = 300 + 20 + 200
    assert r.stdout == "GCF_000001.1_x\t%d\t%d\n" % (L, len(want_bounds(L, 3, 10, 0, k)))
    assert "skipping %s: no valid sequences" % only in r.stderr
    # without the filter every record is joined; the name regexp can be changed
    r = run(["-k", str(k), "-O", str(tmp_path / "o.kmcp"), "--dry-run", "-N", r"^(\w+)_", str(fa), str(only)])
    assert r.returncode == 0, r.stderr
    assert r.stdout == "GCF\t%d\t1\nGCF\t%d\t1\n" % (300 + 20 + 90 + 20 + 200 + 20 + 100, 43)
    # -I / -r
    r = run(["-k", str(k), "-O", str(tmp_path / "o.kmcp"), "--dry-run", "-I", str(tmp_path), "-r", r"\.fna$"])
    assert r.returncode == 0 and r.stdout == "GCF_000002.2\t43\t1\n", r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "o.kmcp")
