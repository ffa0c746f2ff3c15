"""kmcp-refstats --cooccur (cli/kmcp_refstats.cpp: stage 2/4 of `kmcp profile`) against the plain restatement of profile.go:1117-1279
in tests/cooccur_reference.py, on crafted results.  Every case has a pair whose count the quirk it is about changes, and says what the
count is (so neither side can pass on an empty file).

The cases run at --level strain: a reference is kept when it has a unique read of its own (the `u_*` queries); `d1` never has one and is
dropped by stage 1 (verdict no-unique)."""
import gzip
import os
import random
import subprocess
from collections import Counter
from itertools import combinations

import pytest

from tests import cooccur_reference as CR
from tests import filter_cases as FC
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


def keepers(*names, **kw):
    """a unique read for each: stage 1 keeps them"""
    return [row(f"u_{n}", n, **kw) for n in names]


def both(tmp_path, texts, args=(), **kw):
    """the pairs file of the tool on the input files `texts`, held against the restatement's; returns {(refA, refB): reads}"""
    files = []
    for i, t in enumerate(texts):
        files.append(tmp_path / f"in{i}.tsv")
        files[-1].write_text(t)
    ref = CR.cooccur(texts, level="strain", **kw)
    out = tmp_path / "pairs.tsv"
    with_flag = run(["--level", "strain", *args, "--cooccur", out, *files]).stdout
    assert out.read_text() == ref
    assert with_flag == run(["--level", "strain", *args, *files]).stdout  # the stage-1 output is what it is without the flag
    assert ref.startswith(f"# pairs: {len(CR.pairs_of(ref))}\n" + CR.HEADER)
    return CR.pairs_of(ref)


def test_a_query_with_one_target_counts_nothing(tmp_path):
    rows = keepers("a1", "b1") + [row("q", "a1"), row("r", "a1"), row("r", "b1")]
    assert both(tmp_path, ["".join(rows)]) == {("a1", "b1"): 1}


def test_two_rows_of_one_target_are_one_target(tmp_path):
    rows = keepers("b1") + [row("u_a1", "a1", chunk=0, chunks=2), row("q", "a1", chunk=0, chunks=2), row("q", "a1", chunk=1, chunks=2), row("q", "b1")]
    assert both(tmp_path, ["".join(rows)]) == {("a1", "b1"): 1}


def test_a_dropped_target_among_three(tmp_path):
    rows = keepers("a1", "b1") + [row("q", "b1"), row("q", "d1"), row("q", "a1")]
    assert both(tmp_path, ["".join(rows)]) == {("a1", "b1"): 1}  # not (a1, d1), not (b1, d1)


def test_a_dropped_target_does_not_start_a_query(tmp_path):
    # r's rows (two targets, so neither has a unique read) are skipped before the query test: the q rows on both sides of them are ONE
    # query to stage 2
    rows = keepers("a1", "b1") + [row("q", "a1"), row("r", "d1"), row("r", "e1"), row("q", "b1")]
    assert both(tmp_path, ["".join(rows)]) == {("a1", "b1"): 1}
    # ... and as a query's first row it does not make the next row a later one: a1 is q's first kept row, exempt from --keep-perfect-matches;
    # nor does its qCov of 1 become the previous score
    # (to stage 1 the query is its two perfect matches, so neither of them is unique)
    rows = keepers("a1", "b1") + [row("q", "d1", qcov="1.0000"), row("q", "e1", qcov="1.0000"), row("q", "a1", qcov="0.9000"), row("q", "b1", qcov="0.9000")]
    assert both(tmp_path, ["".join(rows)], ["--keep-perfect-matches"], keep_perfect=True) == {("a1", "b1"): 1}


def test_the_gap_of_keep_main_matches_is_taken_to_the_previous_kept_target(tmp_path):
    # q: 1.0 -> (0.7, dropped) -> 0.58: the gap is 0.42 > 0.4, b1 is cut; r: the same scores with a kept target between them
    rows = keepers("a1", "b1", "c1") + [row("q", "a1", qcov="1.0000"), row("q", "d1", qcov="0.7000"), row("q", "b1", qcov="0.5800"),
                                        row("r", "a1", qcov="1.0000"), row("r", "c1", qcov="0.7000"), row("r", "b1", qcov="0.5800")]
    want = {("a1", "b1"): 1, ("a1", "c1"): 1, ("b1", "c1"): 1}
    assert both(tmp_path, ["".join(rows)], ["--keep-main-matches"], keep_main_matches=True) == want
    assert both(tmp_path, ["".join(rows)], ["-m", "0", "-H", "0.75"], mode=0, min_hic_ureads_qcov=0.75) == want
    assert both(tmp_path, ["".join(rows)]) == {**want, ("a1", "b1"): 2}  # without the cut


def test_keep_top_qcovs_with_ties_and_a_dropped_target_between(tmp_path):
    # -n 1: a query's first row counts as one, an equal score is not a smaller one, the next smaller one ends the query
    rows = keepers("a1", "b1", "c1") + [row("q", "a1", qcov="0.9000"), row("q", "b1", qcov="0.9000"), row("q", "c1", qcov="0.8000"), row("q", "a1", qcov="0.9000")]
    assert both(tmp_path, ["".join(rows)], ["-n", "1"], top_n=1) == {("a1", "b1"): 1}
    # -n 2: the dropped target's smaller score is not counted, so b1's is the second
    rows = keepers("a1", "b1", "c1") + [row("q", "a1", qcov="0.9000"), row("q", "d1", qcov="0.8500"), row("q", "b1", qcov="0.8000"), row("q", "c1", qcov="0.7000")]
    assert both(tmp_path, ["".join(rows)], ["-n", "2"], top_n=2) == {("a1", "b1"): 1}


def test_keep_perfect_matches(tmp_path):
    rows = keepers("a1", "b1", "c1") + [row("q", "a1", qcov="1.0000"), row("q", "b1", qcov="1.0000"), row("q", "c1", qcov="0.9000"), row("q", "c1", qcov="1.0000"),
                                        row("r", "b1", qcov="0.9000"), row("r", "c1", qcov="0.8000")]  # no perfect match: everything stays
    assert both(tmp_path, ["".join(rows)], ["--keep-perfect-matches"], keep_perfect=True) == {("a1", "b1"): 1, ("b1", "c1"): 1}


def test_rows_failing_t_or_f_are_gone_before_stage_2(tmp_path):
    rows = keepers("a1", "b1", "c1") + [row("q", "a1"), row("q", "b1", fpr="2.0000e-02"), row("q", "c1", qcov="0.5000"),
                                        row("r", "a1", fpr="1.0000e-02"), row("r", "b1", qcov="0.5500")]  # both boundaries keep
    assert both(tmp_path, ["".join(rows)]) == {("a1", "b1"): 1}
    assert both(tmp_path, ["".join(rows)], ["-f", "1", "-t", "0"], max_fpr=1, min_qcov=0) == {("a1", "b1"): 2, ("a1", "c1"): 1, ("b1", "c1"): 1}


def test_two_input_files_a_query_does_not_span_them_and_gz_output(tmp_path):
    rows = keepers("a1", "b1") + [row("r", "a1"), row("r", "b1"), row("q", "a1"), row("q", "b1")]
    cut = len(rows) - 1
    one, two = ["".join(rows)], ["".join(rows[:cut]), "".join(rows[cut:])]
    assert both(tmp_path, one) == {("a1", "b1"): 2}
    assert both(tmp_path, two) == {("a1", "b1"): 1}
    out, stats = tmp_path / "pairs.tsv.gz", tmp_path / "stats.tsv.gz"
    run(["ref-stats", "--level", "strain", "-o", stats, "--cooccur", out, tmp_path / "in0.tsv", tmp_path / "in1.tsv"])
    assert gzip.open(out, "rt").read() == CR.cooccur(two, level="strain")
    assert gzip.open(stats, "rt").read() == RR.refstats(two, level="strain")
    # the dispatcher's spelling hands the flag on
    out2 = tmp_path / "pairs2.tsv"
    run(["utils", "ref-stats", "--level", "strain", "--cooccur", out2, tmp_path / "in0.tsv", tmp_path / "in1.tsv"], tool=os.path.join(ROOT, "kmcp_amd", "kmcp"))
    assert out2.read_text() == CR.cooccur(two, level="strain")


def test_pairs_are_oriented_and_sorted_by_name(tmp_path):
    # the classes are handed out in order of appearance: z9 first
    rows = keepers("z9", "a1", "m5") + [row("q", "z9"), row("q", "m5"), row("q", "a1"), row("r", "z9"), row("r", "a1")]
    got = both(tmp_path, ["".join(rows)])
    assert list(got.items()) == [(("a1", "m5"), 1), (("a1", "z9"), 2), (("m5", "z9"), 1)]


def test_refusals(tmp_path):
    f = tmp_path / "in.tsv"
    f.write_text(row("q", "a1"))
    s = ["--level", "strain"]
    r = run([*s, "--cooccur", tmp_path / "p.tsv"], expect=255, stdin=b"not a search result\n")  # refused before anything is read
    assert b"stdin is not supported" in r.stderr
    assert b"stdin is not supported" in run([*s, "--cooccur", tmp_path / "p.tsv", f, "-"], expect=255, stdin=b"").stderr
    assert b"must not be the out file" in run([*s, "-o", tmp_path / "o.tsv", "--cooccur", tmp_path / "o.tsv", f], expect=255).stderr
    assert b"must not be the out file" in run([*s, "--cooccur", "-", f], expect=255).stderr  # both on stdout
    assert b"input file" in run([*s, "--cooccur", f, f], expect=255).stderr
    run([*s, "--cooccur"], expect=255)
    assert not (tmp_path / "p.tsv").exists() and not (tmp_path / "o.tsv").exists()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_without_cuts_the_file_is_a_count_over_read_sets_filtered_by_verdict(tmp_path, seed):
    """what kmcp-search --ref-stats-cooccur relies on: with -f 1 -t 0 and no cuts, skipping the dropped targets' rows only takes targets out
    of a query's set — one pass that counts every pair and filters by verdict at the end equals the reference's two passes"""
    rng = random.Random(seed)
    names = [f"t{i}" for i in range(9)]
    chunks = {n: rng.choice([1, 2, 3]) for n in names}
    rows, sets = [], []
    for q in range(120):
        k = rng.choice([1, 1, 2, 3, 5])
        ts = rng.sample(names[:7] if k == 1 else names, k)  # t7 and t8 never have a read of their own: stage 1 drops them
        qrows = [(t, rng.randrange(chunks[t])) for t in ts for _ in range(rng.choice([1, 1, 2]))]
        rng.shuffle(qrows)
        rows += [row(f"q{q}", t, chunk=c, chunks=chunks[t], qcov="%.4f" % rng.choice([0.3, 0.6, 0.74, 0.8, 1.0]), fpr=rng.choice(["1.0000e-03", "5.0000e-01"]))
                 for t, c in qrows]
        sets.append(set(ts))
    text = "".join(rows)
    args = dict(max_fpr=1, min_qcov=0)
    verdicts = RR.verdicts_of(RR.refstats([text], level="strain", **args))
    ok = {n for n, v in verdicts.items() if v == "ok"}
    assert 2 <= len(ok) < len(verdicts)  # some references are dropped, several are kept
    want = Counter()
    for s in sets:
        want.update(combinations(sorted(s & ok), 2))
    assert len(want) >= 2 and max(want.values()) > 1
    assert both(tmp_path, [text], ["-f", "1", "-t", "0"], **args) == dict(want)
