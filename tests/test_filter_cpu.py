"""kmcp-filter (cli/kmcp_filter.cpp: `kmcp utils filter`) against the plain restatement of filter.go in tests/filter_reference.py, which
uses the literal rule (LCA by walking parents, then "at or below species"), on crafted results and the crafted taxdump of
tests/filter_cases.py; and the class shortcut of kmcp_amd/csrc/specific_rule.hpp against the literal rule in a stand-alone program
(tests/specific_rule_check.cpp, built with the address and undefined-behaviour sanitizers)."""
import gzip
import os
import subprocess

import pytest

from tests import filter_cases as FC
from tests import filter_reference as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER = os.path.join(ROOT, "kmcp_amd", "kmcp-filter")
row = FC.row


def run(args, expect=0, stdin=None):
    if not os.path.exists(FILTER):
        import __graft_entry__ as g
        g.build()
    r = subprocess.run([FILTER] + [str(a) for a in args], capture_output=True, input=stdin, timeout=120)
    assert r.returncode == expect, (r.returncode, r.stderr.decode())
    return r


@pytest.fixture(scope="module")
def tax(tmp_path_factory):
    d = tmp_path_factory.mktemp("taxdump")
    return FC.write_taxdump(d / "dump"), FC.write_map(d / "map.tsv")


# (name, rows, kept at species level, kept at strain level) — the expectations are what the restatement must say too
CASES = [
    ("one target in three chunks", [row("q", "a1", chunk=i, chunks=3) for i in range(3)], True, True),
    ("strains, a node below a strain and the species itself", [row("q", t) for t in ("a1", "a2", "a3", "aS")], True, False),
    ("a subspecies and its strain", [row("q", "c1"), row("q", "c2")], True, False),
    ("two species of one genus", [row("q", "a1"), row("q", "b1")], False, False),
    ("a species and one under a species group of the genus", [row("q", "a1"), row("q", "g1")], False, False),
    ("two families", [row("q", "a1"), row("q", "f1")], False, False),
    ("a TaxId above species shared by two targets", [row("q", "x1"), row("q", "x2")], False, False),
    ("a TaxId above species, one target", [row("q", "x1", chunk=0, chunks=2), row("q", "x1", chunk=1, chunks=2)], True, True),
    ("a node with no species above it, one target", [row("q", "x3")], True, True),
    ("a merged TaxId beside a strain of its target's species", [row("q", "m1"), row("q", "a2")], True, False),
    ("a deleted TaxId shared by two targets", [row("q", "d1"), row("q", "d2")], False, False),
    ("a deleted TaxId, one target", [row("q", "d1")], True, True),
    ("an absent TaxId beside a known one", [row("q", "n1"), row("q", "a1")], False, False),
    ("an absent TaxId, one target", [row("q", "n1")], True, True),
    ("-f takes the second species away", [row("q", "a1"), row("q", "b1", fpr="6.0000e-02")], True, True),
    ("-f at the boundary keeps it", [row("q", "a1"), row("q", "b1", fpr="5.0000e-02")], False, False),
    ("-t takes the second species away", [row("q", "a1"), row("q", "c1", qcov="0.5499")], True, True),
    ("0.5500 is not below -t 0.55", [row("q", "a1"), row("q", "c1", qcov="0.5500")], False, False),
    ("every row falls", [row("q", "a1", qcov="0.1000"), row("q", "b1", fpr="0.5")], None, None),
]


@pytest.mark.parametrize("level", ["species", "strain", "assembly"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_single_queries(tax, tmp_path, case, level):
    dump, tmap = tax
    name, rows, keep_species, keep_strain = case
    f = tmp_path / "in.tsv"
    f.write_text("".join(rows))
    verdicts = []
    ref = FR.filter_files([rows], level=level, taxid_map=FR.read_taxid_maps([tmap]), tax=FR.Taxonomy(dump), verdicts=verdicts)
    want = keep_species if level == "species" else keep_strain
    assert [v[2] for v in verdicts] == ([] if want is None else [want]), f"{name}: the restatement's verdict"
    got = run(["--level", level, "-T", tmap, "-X", dump, f]).stdout.decode()
    assert got == ref, name


def all_rows():
    """every case as a query of its own name, comments, blank lines and a query name that comes back later in between"""
    lines = [FR.HEADER]
    for i, (_, rows, _, _) in enumerate(CASES):
        lines += [r.replace("q\t", f"read{i}\t", 1) for r in rows]
        if i % 5 == 2:
            lines += ["\n", "# a comment\n", "#\n"]
    lines += [row("again", "a1"), row("other", "b1"), row("again", "b1"), row("again", "b1", chunk=1, chunks=2)]
    lines += ["# input queries: 40\n", "# matched queries: 23\n", "# matched percentage: 57.5000%\n"]
    return lines


def test_a_whole_file_strain_level_needs_no_taxonomy(tax, tmp_path):
    lines = all_rows()
    f = tmp_path / "in.tsv"
    f.write_text("".join(lines))
    ref = FR.filter_files([lines], level="strain")
    assert run(["--level", "strain", f]).stdout.decode() == ref
    assert run(["filter", "--level", "STRAIN", "--line-chunk-size", "100", "-j", "4", f]).stdout.decode() == ref
    # the same name again after another query is a new query: "again" is judged twice, kept both times (one target each time)
    assert ref.count("again\t") == 3 and "other\t" in ref


def test_a_whole_file_every_form_of_input_and_output(tax, tmp_path):
    dump, tmap = tax
    lines = all_rows()
    half = len(lines) // 2
    tmap_ids, taxo = FR.read_taxid_maps([tmap]), FR.Taxonomy(dump)
    f = tmp_path / "in.tsv"
    f.write_text("".join(lines))
    gz = tmp_path / "in.tsv.gz"
    with gzip.open(gz, "wt") as fh:
        fh.write("".join(lines))
    a, b = tmp_path / "a.tsv", tmp_path / "b.tsv.gz"
    a.write_text("".join(lines[:half]))
    with gzip.open(b, "wt") as fh:
        fh.write("".join(lines[half:]))
    tx = ["-T", tmap, "-X", dump]
    ref = FR.filter_files([lines], taxid_map=tmap_ids, tax=taxo)
    assert ref.count("\n") > 12
    assert run(tx + [f]).stdout.decode() == ref
    assert run(tx + [gz]).stdout.decode() == ref
    assert run(tx, stdin="".join(lines).encode()).stdout.decode() == ref
    assert run(tx + ["-"], stdin=gzip.compress("".join(lines).encode())).stdout.decode() == ref
    # -H, -o plain and .gz
    ref_h = FR.filter_files([lines], taxid_map=tmap_ids, tax=taxo, header=False)
    assert ref_h == ref[len(FR.HEADER):]
    assert run(tx + ["-H", f]).stdout.decode() == ref_h
    o = tmp_path / "out.tsv"
    assert run(tx + ["-o", o, f]).stdout == b"" and o.read_text() == ref
    og = tmp_path / "out.tsv.gz"
    run(tx + ["--out-file", og, "--no-header-row", f])
    assert og.read_bytes()[:2] == b"\x1f\x8b" and gzip.decompress(og.read_bytes()).decode() == ref_h
    # two input files (a query does not go on into the next file), once through -i
    ref2 = FR.filter_files([lines[:half], lines[half:]], taxid_map=tmap_ids, tax=taxo)
    assert run(tx + [a, b]).stdout.decode() == ref2
    lst = tmp_path / "list.txt"
    lst.write_text(f"{a}\n\n{b}\n")
    assert run(tx + ["-i", lst]).stdout.decode() == ref2
    # other thresholds: rows come back and verdicts change
    for fpr, qcov in ((1, 0), (0.06, 0.55), (0.05, 0.9)):
        r = FR.filter_files([lines], max_fpr=fpr, min_qcov=qcov, taxid_map=tmap_ids, tax=taxo)
        assert run(tx + ["-f", fpr, "-t", qcov, f]).stdout.decode() == r
    assert FR.filter_files([lines], max_fpr=1, min_qcov=0, taxid_map=tmap_ids, tax=taxo) != ref
    # a last line without a line end, and \r\n, are written as they are
    odd = [row("q1", "a1", end="\r\n"), row("q1", "a2", end="\r\n"), row("q2", "b1", end="")]
    f2 = tmp_path / "odd.tsv"
    f2.write_bytes("".join(odd).encode())
    assert run(tx + [f2]).stdout.decode() == FR.filter_files([odd], taxid_map=tmap_ids, tax=taxo) == FR.HEADER + "".join(odd)


def test_later_taxid_maps_override_and_comma_lists(tax, tmp_path):
    dump, tmap = tax
    second = tmp_path / "second.tsv"  # b1 moves into species 110; lines without a second column are skipped
    second.write_text("b1\t112\nonly-one-column\n\n")
    rows = [row("q", "a1"), row("q", "b1")]
    f = tmp_path / "in.tsv"
    f.write_text("".join(rows))
    one = FR.filter_files([rows], taxid_map=FR.read_taxid_maps([tmap]), tax=FR.Taxonomy(dump))
    two = FR.filter_files([rows], taxid_map=FR.read_taxid_maps([tmap, second]), tax=FR.Taxonomy(dump))
    assert one == FR.HEADER and two == FR.HEADER + "".join(rows)
    assert run(["-T", tmap, "-X", dump, f]).stdout.decode() == one
    assert run(["-T", tmap, "-T", second, "-X", dump, f]).stdout.decode() == two
    assert run(["--taxid-map", f"{tmap},{second}", "--taxdump", dump, f]).stdout.decode() == two
    assert run(["-T", f"{second},{tmap}", "-X", dump, f]).stdout.decode() == one


def test_unknown_taxids_are_counted_in_one_warning(tax, tmp_path):
    dump, tmap = tax
    f = tmp_path / "in.tsv"
    f.write_text(row("q", "a1"))
    err = run(["-T", tmap, "-X", dump, f]).stderr.decode()
    warn = [l for l in err.splitlines() if l.startswith("[WARN]")]
    assert len(warn) == 1 and warn[0].startswith("[WARN] 2 TaxId(s)"), err  # 888 (deleted) and 777 (absent)


def test_errors(tax, tmp_path):
    dump, tmap = tax
    f = tmp_path / "in.tsv"
    f.write_text(row("q", "a1"))
    tx = ["-T", tmap, "-X", dump]

    def dies(args, message, stdin=None):
        r = run(args, expect=255, stdin=stdin)
        assert r.stdout == b"", r.stdout
        assert r.stderr.decode().splitlines()[-1] == "[ERRO] " + message, r.stderr.decode()

    dies(["--level", "genus", f], "invalid value for --level, available values: species, strain/assembly")
    dies(["-T", tmap, f], "flag -X/--taxdump is needed when -T/--taxid-map given")
    dies(["--level", "strain", "-T", tmap, f], "flag -X/--taxdump is needed when -T/--taxid-map given")
    dies(["-X", dump, f], "flag -T/--taxid-map is needed when -X/--taxdump given")
    dies([f], "TaxID mapping files (-T/--taxid-map) and taxonomy dump files are needed for --level species")
    dies(tx + ["-f", "0", f], "value of flag --max-fpr should be greater than 0")
    dies(tx + ["-t", "-0.1", f], "value of flag --min-query-cov should be greater than or equal to ")
    dies(tx + ["--line-chunk-size", "0", f], "value of flag --line-chunk-size should be greater than 0")
    dies(tx + ["-o", f, f], "out file should not be one of the input file")
    dies(tx + ["-o", f"{tmp_path}//in.tsv", f], "out file should not be one of the input file")
    bad = tmp_path / "bad_map.tsv"
    bad.write_text("a1\t111\nb1\tx12\n")
    dies(["-T", bad, "-X", dump, f], "invalid TaxId: x12")
    bad.write_text("a1\t-5\n")
    dies(["-T", bad, "-X", dump, f], "invalid TaxId: -5")
    empty = tmp_path / "empty_map.tsv"
    empty.write_text("\n")
    dies(["-T", empty, "-X", dump, f], f"no valid TaxIds found in TaxId mapping file: {empty}")
    g = tmp_path / "unknown.tsv"
    g.write_text(row("q", "a1") + row("q2", "zz9"))
    dies(tx + [g], "unknown taxid for zz9, please check taxid mapping file(s)")
    assert run(["--level", "strain"] + tx + [g]).stdout.decode() == FR.HEADER + g.read_text()  # ... at level species only
    with pytest.raises(FR.FilterError, match="unknown taxid for zz9"):
        FR.filter_files([FR.lines_of(g)], taxid_map=FR.read_taxid_maps([tmap]), tax=FR.Taxonomy(dump))
    g.write_text("q\t150\t130\t1e-3\t1\ta1\t0\t1\t30000\t21\t104\t0.8\n")  # 12 fields
    dies(tx + [g], "invalid kmcp search result format")
    g.write_text(row("q", "a1", fpr="abc"))
    dies(tx + [g], "failed to parse FPR: abc")
    g.write_text(row("q", "a1", qcov="0.8x"))
    dies(tx + [g], "failed to parse qCov: 0.8x")
    g.write_text(row("q", "a1", fpr="0.9", qcov="zz"))  # the row falls to -f before its qCov is looked at
    assert run(tx + [g]).stdout.decode() == FR.HEADER
    r = run(["-T", tmap, "-X", tmp_path / "no_such_dir", f], expect=255)
    assert b"err on loading Taxonomy nodes" in r.stderr and r.stdout == b""
    r = run(tx + [tmp_path / "no_such_file.tsv"], expect=255)
    assert b"no_such_file.tsv" in r.stderr and r.stdout == b""
    r = run(tx + ["--no-such-flag", f], expect=255)
    assert b"unknown flag: --no-such-flag" in r.stderr


def test_the_class_shortcut_is_the_literal_rule(tmp_path):
    """tests/specific_rule_check.cpp: a program of its own, with the sanitizers"""
    exe = str(tmp_path / "specific_rule_check")
    src = [os.path.join(ROOT, "tests", "specific_rule_check.cpp"), os.path.join(ROOT, "kmcp_amd", "csrc", "taxonomy.cpp")]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe] + src, check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
