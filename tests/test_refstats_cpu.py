"""kmcp-refstats (cli/kmcp_refstats.cpp: stage 1/4 of `kmcp profile`) against the plain restatement of profile.go in
tests/refstats_reference.py, on crafted results and the crafted taxdump of tests/filter_cases.py."""
import gzip
import os
import subprocess

import pytest

from tests import filter_cases as FC
from tests import filter_reference as FR
from tests import refstats_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "kmcp_amd", "kmcp-refstats")
row = FC.row


def run(args, expect=0, stdin=None, tool=TOOL):
    if not os.path.exists(tool):
        import __graft_entry__ as g
        g.build()
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, input=stdin, timeout=120)
    assert r.returncode == expect, (r.returncode, r.stderr.decode())
    return r


@pytest.fixture(scope="module")
def tax(tmp_path_factory):
    d = tmp_path_factory.mktemp("taxdump")
    dump, tmap = FC.write_taxdump(d / "dump"), FC.write_map(d / "map.tsv")
    return dump, tmap, FR.read_taxid_maps([tmap]), FR.Taxonomy(dump)


def both(tax, tmp_path, rows, level, args=(), **kw):
    """the tool's output on `rows`, held against the restatement's"""
    dump, tmap, ids, taxo = tax
    f = tmp_path / "in.tsv"
    f.write_text("".join(rows))
    ref = RR.refstats(["".join(rows)], level=level, taxid_map=ids, tax=taxo, **kw)
    got = run(["--level", level, "-T", tmap, "-X", dump, *args, f]).stdout.decode()
    assert got == ref
    return {l.split("\t")[0]: l.rstrip("\n").split("\t")[1:] for l in got.splitlines() if l[0] != "#"}, got


def test_one_target_one_chunk(tax, tmp_path):
    refs, got = both(tax, tmp_path, [row("q", "a1")], "species")
    assert refs == {"a1": ["1", "30000", "1", "1", "1", "1.0000", "ok", "1", "1", "1", "1"]}
    assert got.startswith("# matched reads: 1\n# unique reads: 1\n" + RR.HEADER)


@pytest.mark.parametrize("level", ["species", "strain"])
def test_one_target_several_chunks_the_first_row_decides(tax, tmp_path, level):
    rows = [row("q", "a1", chunk=2, chunks=4, qcov="0.9000"), row("q", "a1", chunk=0, chunks=4, qcov="0.6000"), row("q", "a1", chunk=2, chunks=4, qcov="0.5600")]
    refs, _ = both(tax, tmp_path, rows, level)
    assert refs["a1"][7:] == ["1,0,2,0", "0,0,1,0", "0,0,1,0", "0,0,1,0"] and refs["a1"][5:7] == ["0.5000", "low-chunks-fraction"]


@pytest.mark.parametrize("level,second,unique", [("species", "a2", True), ("strain", "a2", False), ("species", "b1", False), ("strain", "b1", False)])
def test_two_targets(tax, tmp_path, level, second, unique):
    refs, got = both(tax, tmp_path, [row("q", "a1"), row("q", second)], level)
    assert f"# unique reads: {int(unique)}\n" in got
    assert refs["a1"][2:5] == ["1", str(int(unique)), str(int(unique))] and refs["a1"][6] == ("ok" if unique else "no-unique")
    assert refs[second][2:5] == refs["a1"][2:5]


def test_a_second_row_with_the_higher_chunk_index(tax, tmp_path):
    rows = [row("q", "a1", chunk=0, chunks=3), row("q", "a2", chunk=1, chunks=2), row("q", "a1", chunk=2, chunks=3), row("q", "a2", chunk=0, chunks=2)]
    refs, _ = both(tax, tmp_path, rows, "species")
    assert refs["a1"][7:] == ["1,0,1", "1,0,0", "1,0,0", "1,0,0"] and refs["a2"][7:] == ["1,1", "0,1", "0,1", "0,1"]


def test_rows_dropped_by_f_and_t(tax, tmp_path):
    rows = [row("e", "a1", qcov="0.5499"), row("e", "b1", fpr="2.0000e-02"),                       # an empty query
            row("s", "a1"), row("s", "b1", fpr="1.0001e-02"), row("s", "c1", qcov="0.1000"),        # left single-target
            row("k", "a1", fpr="1.0000e-02"), row("k", "b1", qcov="0.5500")]                        # both boundaries keep
    refs, got = both(tax, tmp_path, rows, "species")
    assert "# matched reads: 2\n# unique reads: 1\n" in got and refs["a1"][2:4] == ["2", "1"] and refs["b1"][2:4] == ["1", "0"] and "c1" not in refs


@pytest.mark.parametrize("qcov,hic", [("0.7500", 1), ("0.7499", 0)])
def test_qcov_at_H_and_one_printed_digit_below(tax, tmp_path, qcov, hic):
    refs, _ = both(tax, tmp_path, [row("q", "a1", qcov=qcov)], "strain")
    assert refs["a1"][4] == str(hic) and refs["a1"][6] == ("ok" if hic else "no-hic-unique")


def test_keep_top_qcovs(tax, tmp_path):
    # -n 1: the rows of the best qCov only (equal scores do not count as a smaller one); the cut ends the query
    rows = [row("q", "a1", qcov="0.9000"), row("q", "a2", qcov="0.9000"), row("q", "b1", qcov="0.8000"), row("q", "c1", qcov="0.8000"),
            row("r", "b1", qcov="0.7000")]
    refs, got = both(tax, tmp_path, rows, "species", ["-n", "1"], top_n=1)
    assert set(refs) == {"a1", "a2", "b1"} and "# matched reads: 2\n# unique reads: 2\n" in got
    refs, _ = both(tax, tmp_path, rows, "species", ["-n", "2"], top_n=2)
    assert set(refs) == {"a1", "a2", "b1", "c1"}


def test_keep_perfect_matches(tax, tmp_path):
    rows = [row("q", "a1", qcov="1.0000"), row("q", "a2", qcov="1.0000"), row("q", "b1", qcov="0.9000"), row("q", "c1", qcov="1.0000"),
            row("r", "b1", qcov="0.9000"), row("r", "c1", qcov="0.8000")]  # no perfect match: everything stays
    refs, got = both(tax, tmp_path, rows, "species", ["--keep-perfect-matches"], keep_perfect=True)
    assert refs["a1"][3] == "1" and refs["b1"][2:4] == ["1", "0"] and refs["c1"][2] == "1" and "# unique reads: 1\n" in got


def test_mode_0_gap_cut_and_the_first_row_exemption(tax, tmp_path):
    # the gap is taken to the previous KEPT row; a query's first row is never tested, whatever the previous query's last score was
    rows = [row("q", "a1", qcov="1.0000"), row("q", "a2", qcov="0.6100"), row("q", "b1", qcov="0.2000"), row("q", "c1", qcov="0.6000"),
            row("r", "f1", qcov="0.1500"), row("r", "c1", qcov="0.1000")]
    refs, got = both(tax, tmp_path, rows, "species", ["-m", "0", "-t", "0.1"], mode=0, min_qcov=0.1)
    assert set(refs) == {"a1", "a2", "f1", "c1"} and refs["c1"][2] == "1" and "# matched reads: 2\n" in got
    refs2, _ = both(tax, tmp_path, rows, "species", ["--keep-main-matches", "-t", "0.1", "--max-qcov-gap", "0.38"], keep_main_matches=True, min_qcov=0.1, max_gap=0.38)
    assert set(refs2) == {"a1", "f1", "c1"}
    refs3, _ = both(tax, tmp_path, rows, "species", ["-t", "0.1"], min_qcov=0.1)
    assert set(refs3) == {"a1", "a2", "b1", "c1", "f1"}


def test_adjacent_queries_of_one_name_merge_and_a_name_that_returns_does_not(tax, tmp_path):
    rows = [row("q", "a1", qidx=0), row("q", "b1", qidx=1), row("o", "a1"), row("q", "a1")]
    refs, got = both(tax, tmp_path, rows, "species")
    assert "# matched reads: 3\n# unique reads: 2\n" in got and refs["a1"][2:4] == ["3", "2"]


def whole_file():
    lines = [FR.HEADER]
    for i, t in enumerate(["a1", "a1", "a2", "b1", "c1", "c2", "f1"]):
        lines += [row(f"read{i}", t, chunk=i % 3, chunks=3, qcov="0.%d000" % (6 + i % 4))]
        if i % 2:
            lines += [row(f"read{i}", "a3", chunk=1, chunks=2, qcov="0.5600"), "\n", "# a comment\n"]
    lines += ["# input queries: 40\n"]
    return lines


def test_two_input_files_gz_stdin_the_list_file_and_the_dispatcher(tax, tmp_path):
    dump, tmap, ids, taxo = tax
    lines = whole_file()
    half = 3  # cuts read1's two rows apart: a query does not span files
    a, b = tmp_path / "a.tsv", tmp_path / "b.tsv.gz"
    a.write_text("".join(lines[:half]))
    with gzip.open(b, "wt") as fh:
        fh.write("".join(lines[half:]))
    tx = ["-T", tmap, "-X", dump]
    ref2 = RR.refstats(["".join(lines[:half]), "".join(lines[half:])], taxid_map=ids, tax=taxo)
    ref1 = RR.refstats(["".join(lines)], taxid_map=ids, tax=taxo)
    assert ref1 != ref2
    assert run([*tx, a, b]).stdout.decode() == ref2
    lst = tmp_path / "list.txt"
    lst.write_text(f"{a}\n\n{b}\n")
    assert run([*tx, "-i", lst, "--line-chunk-size", "10", "-j", "4"]).stdout.decode() == ref2
    assert run([*tx], stdin="".join(lines).encode()).stdout.decode() == ref1
    out = tmp_path / "o.tsv.gz"
    run(["ref-stats", *tx, "-o", out, a, b])
    assert gzip.open(out, "rt").read() == ref2
    assert run(["utils", "ref-stats", *tx, a, b], tool=os.path.join(ROOT, "kmcp_amd", "kmcp")).stdout.decode() == ref2
    run([*tx, "-o", a, a], expect=255)


def test_a_missing_taxid_is_fatal_at_level_species_only(tax, tmp_path):
    dump, tmap, ids, taxo = tax
    f = tmp_path / "in.tsv"
    f.write_text(row("q", "nobody"))
    r = run(["-T", tmap, "-X", dump, f], expect=255)
    assert b"unknown taxid for nobody" in r.stderr
    with pytest.raises(RR.RefstatsError):
        RR.refstats([row("q", "nobody")], taxid_map=ids, tax=taxo)
    assert run(["--level", "strain", f]).stdout.decode() == RR.refstats([row("q", "nobody")], level="strain")


def test_flag_validation(tax, tmp_path):
    dump, tmap, _, _ = tax
    f = tmp_path / "in.tsv"
    f.write_text(row("q", "a1"))
    s = ["--level", "strain"]
    for bad in (["-m", "6"], ["-m", "-1"], ["-f", "0"], ["-t", "-0.1"], ["-n", "-1"], ["-p", "1.5"], ["-p", "-0.1"], ["-H", "0"], ["-H", "1.01"],
                ["-H", "0.5"],                    # below -t 0.55
                ["-t", "0.8"],                    # the flag's default 0.75 is below -t, as in the reference
                ["-t", "0.8", "-m", "4"],         # ... whatever the mode's own H
                ["--level", "genus"], ["--bogus"], ["-m"], ["-H", "x"]):
        run([*s, *bad, f], expect=255)
    run([f], expect=255)                          # --level species needs -T
    run(["-T", tmap, f], expect=255)
    run(["-X", dump, "--level", "strain", f], expect=255)
    run([*s, tmp_path / "none.tsv"], expect=255)
    f.write_text("q\t1\t2\n")
    run([*s, f], expect=255)                      # fewer than 13 fields
    f.write_text(row("q", "a1", chunk=1, chunks=1))
    run([*s, f], expect=255)                      # a chunk index outside the reference
    f.write_text(row("q", "a1", chunk=0, chunks=1 << 40))
    assert b"at most 65535" in run([*s, f], expect=255).stderr  # a corrupt IdxNum is an error message, not an allocation
    f.write_text(row("q", "a1").replace("\t150\t", "\t15x\t"))
    run([*s, f], expect=255)
    run([*s, "-t", "0.8", "-H", "0.8", "-h"])


@pytest.mark.parametrize("mode", range(6))
def test_every_modes_preset_and_explicit_flags(tax, tmp_path, mode):
    h, p, main = RR.PRESETS[mode]
    chunks = 10
    covered = int(round(p * chunks))
    rows = []
    for name, ncov, qcov in (("a1", covered, h), ("b1", covered - 1, h), ("c1", chunks, h - 0.0001)):
        rows += [row(f"{name}.{c}", name, chunk=c, chunks=chunks, qcov="%.4f" % qcov) for c in range(ncov)]
    rows += [row("g", "f1", qcov="0.9000"), row("g", "a1", qcov="0.4500", chunks=chunks)]  # cut by mode 0's gap only
    refs, _ = both(tax, tmp_path, rows, "species", ["-m", mode, "-t", "0.4"], mode=mode, min_qcov=0.4)
    assert refs["a1"][6] == "ok" and refs["b1"][6] == "low-chunks-fraction" and refs["c1"][6] == "no-hic-unique"
    assert refs["f1"][6] == ("ok" if main else "no-unique")
    # explicit flags override the preset, each alone
    refs, _ = both(tax, tmp_path, rows, "species", ["-m", mode, "-t", "0.4", "-H", "0.6"], mode=mode, min_qcov=0.4, min_hic_ureads_qcov=0.6)
    assert refs["c1"][6] == "ok" and refs["b1"][6] == "low-chunks-fraction"
    refs, _ = both(tax, tmp_path, rows, "species", ["-m", mode, "-t", "0.4", "-p", "0.1"], mode=mode, min_qcov=0.4, min_chunks_fraction=0.1)
    assert refs["b1"][6] == "ok" and refs["c1"][6] == "no-hic-unique"
