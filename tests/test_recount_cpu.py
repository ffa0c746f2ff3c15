"""kmcp-refstats --recount (cli/kmcp_refstats.cpp: stage 3/4 of `kmcp profile`) against the plain restatement of profile.go:1282-1888 in
tests/recount_reference.py, on crafted results.  Verdicts and the three '#' lines must be equal; counts are compared as numbers.

The tolerance is derived, not measured.  The tool adds integer shares of 720720 = lcm(1..16): for a target with m | 720720 rows its count
is the exact rational, the restatement's float64 sum of n terms is off by at most n * 2^-53 relative, so the two agree to the %.6f print:
1e-6 absolute.  A row's bases are floor(qlen * 2^16 / (ns * m)) / 2^16, at most 2^-16 below the restatement's: bases differ by at most
rows * 2^-16 plus the %.4f print; coverage and depthStdev follow from the bases (`compare`).  The 17-row case is held against the exact
fractions of the rule, not the float sum.  The cases' thresholds leave no verdict within those bounds of its cut.

Unless a case says otherwise it runs at --level strain with -r 1 -u 1 -U 1 -P 0.01 -d 10: a reference is kept by stage 1 when it has a
unique read of its own (the `u_*` queries)."""
import gzip
import os
import subprocess
from fractions import Fraction

import pytest

from tests import filter_cases as FC
from tests import filter_reference as FR
from tests import cooccur_reference as CR
from tests import recount_reference as R3
from tests import refstats_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "kmcp_amd", "kmcp-refstats")
LOOSE = ["-r", "1", "-u", "1", "-U", "1", "-P", "0.01", "-d", "10"]
LOOSE_KW = dict(r=1, u=1, U=1, P=0.01, d=10)


def row(query, target, qcov="0.8000", chunk=0, chunks=1, qlen=150, fpr="1.0000e-03", tlen=30000):
    return "\t".join([query, str(qlen), "130", fpr, "1", target, str(chunk), str(chunks), str(tlen), "21", "104", qcov, "0.0100", "0.0100", "0"]) + "\n"


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


def compare(got, ref, n_rows):
    """a recount file of the tool against the restatement's, within the module docstring's bounds; n_rows: the rows of the input"""
    (gh, g), (rh, r) = R3.parse(got), R3.parse(ref)
    assert gh == rh
    assert {k: v["verdict"] for k, v in g.items()} == {k: v["verdict"] for k, v in r.items()}
    eps_b = n_rows * 2.0 ** -16
    for name in r:
        a, b = g[name], r[name]
        assert (a["chunks"], a["tlen"]) == (b["chunks"], b["tlen"])
        for k in range(3):  # reads, ureads, hicUreads and their per-chunk lists
            assert abs(a["numbers"][k] - b["numbers"][k]) <= 1e-6 + 1e-12, (name, k, a["numbers"], b["numbers"])
            assert all(abs(x - y) <= 1e-6 + 1e-12 for x, y in zip(a["lists"][k], b["lists"][k])), (name, k)
        assert a["numbers"][3] == b["numbers"][3]  # chunksFrac: a ratio of small integers
        assert all(abs(x - y) <= eps_b + 1e-4 + 1e-9 for x, y in zip(a["lists"][3], b["lists"][3])), (name, a["lists"][3], b["lists"][3])
        qlens = sum(b["lists"][3])
        assert abs(a["numbers"][4] - b["numbers"][4]) <= 4 * a["chunks"] * eps_b / qlens + 1e-6 + 1e-9  # depthStdev
        assert abs(a["numbers"][5] - b["numbers"][5]) <= a["chunks"] * eps_b / a["tlen"] + 1e-6 + 1e-9  # coverage
    return g


def both(tmp_path, texts, args=LOOSE, level="strain", tax=None, **kw):
    """the recount file of the tool on the input files `texts`, held against the restatement's; the stage-1 and --cooccur outputs are what
    they are without the flag"""
    files = []
    for i, t in enumerate(texts):
        files.append(tmp_path / f"in{i}.tsv")
        files[-1].write_text(t)
    tx, tkw = [], {}
    if tax:
        tx, tkw = ["-T", tax[1], "-X", tax[0]], dict(taxid_map=tax[2], tax=tax[3])
    kw = {**(LOOSE_KW if list(args[:len(LOOSE)]) == LOOSE else {}), **kw}
    ref = R3.recount(texts, level=level, **tkw, **kw)
    out, pairs = tmp_path / "recount.tsv", tmp_path / "pairs.tsv"
    base = ["--level", level, *tx, *args]
    with_flag = run([*base, "--recount", out, "--cooccur", pairs, *files]).stdout
    with_pairs = pairs.read_bytes()
    alone = tmp_path / "recount_alone.tsv"
    assert run([*base, "--recount", alone, *files]).stdout == with_flag  # the pair table is computed whether or not --cooccur is given
    assert alone.read_bytes() == out.read_bytes()
    assert run([*base, "--cooccur", pairs, *files]).stdout == with_flag and pairs.read_bytes() == with_pairs
    return compare(out.read_text(), ref, sum(t.count("\n") for t in texts)), out.read_text()


def uniques(name, n, **kw):
    return [row(f"u_{name}_{i}", name, **kw) for i in range(n)]


QUIRK_ARGS = [*LOOSE, "-D", "0.9", "-R", "0.5"]
QUIRK_KW = dict(LOOSE_KW, min_dreads_prop=0.9, max_mismatch_err=0.5)


def quirk_rows():
    """a1, b1, c1 with 12, 25 and 1 unique reads, two reads shared by b1 and c1, and q naming all three in qCov order.  With D = 0.9 and
    R = 0.5: (a1, b1): 13 * 0.1 >= 1 but 25 < 6 is false; 28 * 0.1 >= 1 and 12 < 12.5: a1 goes.  (a1, c1), in the SAME row: 1.3 >= 1 and
    1 < 6: c1 goes.  (b1, c1) would not: 2.8 >= 3 is false, and 0.4 >= 3 is false."""
    rows = uniques("a1", 12) + uniques("b1", 25) + uniques("c1", 1)
    rows += [row("s1", "b1"), row("s1", "c1"), row("s2", "c1"), row("s2", "b1")]
    return rows + [row("q", "a1", qcov="0.9000"), row("q", "b1", qcov="0.8500"), row("q", "c1", qcov="0.8000")]


def test_the_quirk_case_row_a_goes_on_after_a_is_deleted(tmp_path):
    g, text = both(tmp_path, ["".join(quirk_rows())], QUIRK_ARGS, **QUIRK_KW)
    assert text.startswith("# recounted reads: 41\n# unique reads: 39\n# corrected reads: 1\n" + R3.HEADER)
    # q went to b1 alone ({b1, c1} would give b1 25 + 1 + 1.5 and c1 2.5)
    assert g["b1"]["numbers"][:2] == [28.0, 26.0] and g["a1"]["numbers"][:2] == [12.0, 12.0] and g["c1"]["numbers"][:2] == [3.0, 1.0]
    # without the correction q is shared by three
    g, text = both(tmp_path, ["".join(quirk_rows())], [*QUIRK_ARGS, "--no-amb-corr"], no_amb_corr=True, **QUIRK_KW)
    assert "# unique reads: 38\n# corrected reads: 0\n" in text
    assert g["b1"]["numbers"][0] == 28.0 and g["c1"]["numbers"][0] == 4.0 and g["a1"]["numbers"][0] == 13.0
    assert g["a1"]["lists"][3] == [12 * 150 + 50.0]  # q's 150 bases over three survivors


def test_the_bound_of_max_mismatch_err_is_strict_and_a_pair_without_reads_is_never_asked(tmp_path):
    """r names a1 and b1.  With the defaults (n + 1) * 0.95 >= 1, and b1 goes when 1 < n * 0.05: not at 20 unique reads of a1, at 21.
    (On this route a pair that a read asks for is never absent from stage 2's table — both stages keep the same rows, so the read itself
    is in its count; the absent pair, shared = 0, is a case of tests/recount_rule_check.cpp and of the library's tests.)"""
    for n, lost in ((20, 0), (21, 1)):
        rows = uniques("a1", n) + uniques("b1", 1) + [row("r", "a1"), row("r", "b1")]
        g, text = both(tmp_path, ["".join(rows)])
        assert f"# corrected reads: {lost}\n" in text
        assert g["b1"]["numbers"][0] == (1.0 if lost else 2.0)  # (a surviving target counts the read whole: only the bases are split)
        assert CR.pairs_of((tmp_path / "pairs.tsv").read_text()) == {("a1", "b1"): 1}
    # two references that never meet: nothing to correct
    rows = uniques("a1", 30) + uniques("b1", 1)
    assert "# recounted reads: 31\n# unique reads: 31\n# corrected reads: 0\n" in both(tmp_path, ["".join(rows)])[1]


def test_ties_in_qcov_keep_the_order_of_the_first_rows(tmp_path):
    """x1, y1, z1 with 3, 7 and 1 unique reads, nine reads shared by y1 and z1, R = 0.5, D = 0.5.  y1 beats x1 (3 < 3.5), x1 beats z1
    (1 < 1.5), and neither of y1 and z1 beats the other: they share 10 reads, above 17 * 0.5 and 11 * 0.5.  q names all three at ONE printed
    qCov, so the order is the rows':  x1 y1 z1 -> row x1 deletes z1 and x1: {y1};  y1 x1 z1 -> row y1 deletes x1 only: {y1, z1};
    z1 x1 y1 -> row z1 deletes z1, row x1 deletes x1: {y1}.  A higher qCov moves a target to the front whatever its row."""
    base = uniques("x1", 3) + uniques("y1", 7) + uniques("z1", 1) + [r for i in range(9) for r in (row(f"s{i}", "y1"), row(f"s{i}", "z1"))]
    args, kw = [*LOOSE, "-R", "0.5", "-D", "0.5"], dict(max_mismatch_err=0.5, min_dreads_prop=0.5)
    cases = [(("x1", "y1", "z1"), {}, 10.0), (("y1", "x1", "z1"), {}, 11.0), (("z1", "x1", "y1"), {}, 10.0),
             (("y1", "x1", "z1"), {"x1": "0.8001"}, 10.0), (("x1", "y1", "z1"), {"y1": "0.9000"}, 11.0)]
    for order, qcovs, z_reads in cases:
        rows = base + [row("q", t, qcov=qcovs.get(t, "0.8000")) for t in order]
        g, _ = both(tmp_path, ["".join(rows)], args, **kw)
        assert g["z1"]["numbers"][0] == z_reads and g["y1"]["numbers"][0] == 17.0 and g["x1"]["numbers"][0] == 3.0, (order, qcovs)


def test_a_read_that_is_unique_only_because_stage_1_dropped_its_other_target(tmp_path):
    # d1 has no unique read: stage 1 drops it, its row is skipped, q is a unique read of a1 in stage 3 (stage 1 did not count it as one)
    rows = uniques("a1", 2) + [row("q", "d1", qcov="0.9500"), row("q", "a1", qcov="0.9000")]
    g, text = both(tmp_path, ["".join(rows)])
    assert "# recounted reads: 3\n# unique reads: 3\n# corrected reads: 0\n" in text
    assert g["a1"]["numbers"][:3] == [3.0, 3.0, 3.0] and "d1" not in g
    stage1 = run(["--level", "strain", tmp_path / "in0.tsv"]).stdout.decode()
    assert "a1\t1\t30000\t3\t2\t2\t" in stage1


def test_survivors_under_one_species_add_their_share_to_uniq(tax, tmp_path):
    # a1 and a2 are strains of species 110, b1 of 120.  q: a1 (two rows) and a2: one species -> the first rows add 1/2 and 1 to uniq;
    # hic by the first row's own qCov.  r: a1 and b1: two species -> nothing
    rows = uniques("a1", 1) + uniques("a2", 1) + uniques("b1", 1)
    rows += [row("q", "a1", qcov="0.7000", chunk=0, chunks=2), row("q", "a2", qcov="0.9000"), row("q", "a1", qcov="0.9000", chunk=1, chunks=2)]
    rows += [row("r", "a1", chunk=0, chunks=2), row("r", "b1")]
    rows[0] = row("u_a1_0", "a1", chunk=1, chunks=2)
    g, _ = both(tmp_path, ["".join(rows)], [*LOOSE, "-p", "0"], level="species", tax=tax, min_chunks_fraction=0)
    assert g["a1"]["lists"][1] == [0.5, 1.0] and g["a1"]["lists"][2] == [0.0, 1.0] and g["a2"]["lists"][1] == [2.0] and g["a2"]["lists"][2] == [2.0]
    assert g["a1"]["lists"][3] == [150 / 4 + 75.0, 150 + 150 / 4]
    g, _ = both(tmp_path, ["".join(rows)], [*LOOSE, "-p", "0"], level="strain", min_chunks_fraction=0)
    assert g["a1"]["lists"][1] == [0.0, 1.0] and g["a2"]["lists"][1] == [1.0]


def test_a_target_with_17_rows_the_first_row_takes_the_remainder(tmp_path):
    rows = [row("q", "a1", chunk=c, chunks=17, qlen=170) for c in range(17)]
    out = tmp_path / "r.tsv"
    f = tmp_path / "in.tsv"
    f.write_text("".join(rows))
    run(["--level", "strain", *LOOSE, "--recount", out, f])
    _, g = R3.parse(out.read_text())
    share = 720720 // 17
    exact = [Fraction(720720 - 16 * share, 720720)] + [Fraction(share, 720720)] * 16
    assert sum(exact) == 1
    assert g["a1"]["lists"][0] == [float("%.6f" % float(x)) for x in exact]
    assert g["a1"]["numbers"][:3] == [1.0, 1.0, 1.0] and g["a1"]["lists"][1] == [1.0] + [0.0] * 16
    assert g["a1"]["lists"][3] == [10.0] * 17 and g["a1"]["verdict"] == "low-chunks-fraction"  # (no chunk has -r 1 reads)
    # (the restatement's 17 times 1/17 lies 6.6e-6 from the first row's share and 9e-9 from the others': the remainder is the rule's)
    _, r = R3.parse(R3.recount(["".join(rows)], level="strain", **LOOSE_KW))
    assert r["a1"]["verdict"] == "low-chunks-fraction" and abs(r["a1"]["numbers"][0] - 1.0) <= 1e-6
    assert all(abs(x - y) <= 1e-6 + 1e-12 for x, y in zip(g["a1"]["lists"][0][1:], r["a1"]["lists"][0][1:]))


def test_switches_keep_main_top_n_with_a_skipped_row_in_front_and_two_files(tmp_path):
    base = uniques("a1", 2) + uniques("b1", 2) + uniques("c1", 2)
    # the gap of --keep-main-matches is taken to the previous KEPT target's row: 1.0 -> (0.7, dropped) -> 0.58 cuts b1
    rows = base + [row("q", "a1", qcov="1.0000"), row("q", "d1", qcov="0.7000"), row("q", "b1", qcov="0.5800"),
                   row("r", "a1", qcov="1.0000"), row("r", "c1", qcov="0.7000"), row("r", "b1", qcov="0.5800")]
    g, _ = both(tmp_path, ["".join(rows)], [*LOOSE, "--keep-main-matches"], keep_main_matches=True)
    assert g["a1"]["numbers"][:2] == [4.0, 3.0] and g["b1"]["numbers"][0] == 3.0  # q is a unique read of a1
    g, _ = both(tmp_path, ["".join(rows)])
    assert g["a1"]["numbers"][:2] == [4.0, 2.0] and g["b1"]["numbers"][0] == 4.0
    # -n 1 with a skipped row in front (d1: one of two chunks, low-chunks-fraction; to stage 1 q is d1's read alone): d1's 0.95 is not the
    # first score, a1 and b1 tie at 0.9, c1's 0.8 ends the query
    rows = base + [row("q", "d1", qcov="0.9500", chunks=2), row("q", "a1", qcov="0.9000"), row("q", "b1", qcov="0.9000"), row("q", "c1", qcov="0.8000")]
    g, _ = both(tmp_path, ["".join(rows)], [*LOOSE, "-n", "1"], top_n=1)
    assert g["a1"]["numbers"][0] == 3.0 and g["b1"]["numbers"][0] == 3.0 and g["c1"]["numbers"][0] == 2.0
    assert g["a1"]["lists"][3] == [2 * 150 + 75.0]
    # two input files: a query does not span them
    rows = base + [row("q", "a1"), row("q", "b1")]
    one, two = ["".join(rows)], ["".join(rows[:-1]), "".join(rows[-1:])]
    assert both(tmp_path, one)[0]["a1"]["numbers"][:2] == [3.0, 2.0]
    assert both(tmp_path, two)[0]["a1"]["numbers"][:2] == [3.0, 3.0]


def test_every_verdict_of_stage_3(tmp_path):
    """-r 2 -u 3 -U 2 -P 0.5 -p 1 -d 0.5, every reference with two chunks (stage 1 runs with -p 1 as well: both chunks have a row)"""
    def ref(name, n0, n1, hic, q0=100, q1=100):
        """n0 / n1 unique reads on chunk 0 / 1, the first `hic` of them with a high qCov"""
        out = []
        for i in range(n0 + n1):
            out.append(row(f"u_{name}_{i}", name, chunk=0 if i < n0 else 1, chunks=2, qcov="0.9000" if i < hic else "0.6000", qlen=q0 if i < n0 else q1))
        return out
    rows = ref("few1", 1, 1, 2) + ref("hic1", 2, 2, 1) + ref("prop1", 3, 2, 2) + ref("chunk1", 3, 1, 3) + ref("stdev1", 2, 2, 4, q0=301, q1=99) + ref("ok1", 2, 2, 2, q0=300, q1=100)
    args = ["-r", "2", "-u", "3", "-U", "2", "-P", "0.5", "-p", "1", "-d", "0.5"]
    g, _ = both(tmp_path, ["".join(rows)], args, r=2, u=3, U=2, P=0.5, d=0.5, min_chunks_fraction=1)
    assert {k: v["verdict"] for k, v in g.items()} == {"few1": "few-unique", "hic1": "few-hic-unique", "prop1": "low-hic-unique-prop", "chunk1": "low-chunks-fraction",
                                                       "stdev1": "high-depth-stdev", "ok1": "ok"}
    assert g["ok1"]["numbers"][3:] == [1.0, 0.5, 0.026667] and g["chunk1"]["numbers"][3] == 0.5
    for norm, cov in (("min", 2 * 200 / 30000), ("max", 2 * 600 / 30000)):
        g, _ = both(tmp_path, ["".join(rows)], [*args, "--norm-abund", norm], r=2, u=3, U=2, P=0.5, d=0.5, min_chunks_fraction=1, norm=norm)
        assert g["ok1"]["numbers"][5] == float("%.6f" % cov)
    # the thresholds come from -m when the flags are not given: mode 0 asks 1 1 1 0.01 10 (and -p 0.2)
    g, _ = both(tmp_path, ["".join(rows)], ["-m", "0", "-H", "0.75"], mode=0, min_hic_ureads_qcov=0.75)
    assert set(v["verdict"] for v in g.values()) == {"ok"}
    g, _ = both(tmp_path, ["".join(rows)], ["-m", "0", "-H", "0.75", "-u", "5"], mode=0, min_hic_ureads_qcov=0.75, u=5)
    assert g["few1"]["verdict"] == "few-unique" and g["prop1"]["verdict"] == "ok"


def test_gz_output_the_dispatcher_and_refusals(tmp_path):
    rows = quirk_rows()
    f = tmp_path / "in.tsv"
    f.write_text("".join(rows))
    s = ["--level", "strain", *QUIRK_ARGS]
    plain, gz = tmp_path / "r.tsv", tmp_path / "r.tsv.gz"
    run([*s, "--recount", plain, f])
    run(["ref-stats", *s, "--recount", gz, "-o", tmp_path / "o.tsv.gz", f])
    assert gzip.open(gz, "rt").read() == plain.read_text()
    assert gzip.open(tmp_path / "o.tsv.gz", "rt").read() == RR.refstats(["".join(rows)], level="strain")
    via = tmp_path / "via.tsv"
    run(["utils", "ref-stats", *s, "--recount", via, f], tool=os.path.join(ROOT, "kmcp_amd", "kmcp"))
    assert via.read_bytes() == plain.read_bytes()
    # refused with status 255 before anything is read
    p = tmp_path / "p.tsv"
    t = ["--level", "strain"]
    assert b"stdin is not supported" in run([*t, "--recount", p], expect=255, stdin=b"not a search result\n").stderr
    assert b"stdin is not supported" in run([*t, "--recount", p, f, "-"], expect=255, stdin=b"").stderr
    assert b"must not be the out file" in run([*t, "-o", p, "--recount", p, f], expect=255).stderr
    assert b"must not be the out file" in run([*t, "--recount", "-", f], expect=255).stderr
    assert b"--cooccur file" in run([*t, "--cooccur", p, "--recount", p, f], expect=255).stderr
    assert b"input file" in run([*t, "--recount", f, f], expect=255).stderr
    for bad in (["-r", "0"], ["-u", "0"], ["-U", "-1"], ["-P", "1.5"], ["-P", "0"], ["-d", "0"], ["-D", "0"], ["-D", "1.5"], ["-R", "1"], ["-R", "0"], ["--norm-abund", "median"],
                ["-r", "x"], ["--recount"]):
        run([*t, *bad, "--recount", p, f] if bad != ["--recount"] else [*t, f, "--recount"], expect=255)
    assert not p.exists()
    assert f.read_text() == "".join(rows)
