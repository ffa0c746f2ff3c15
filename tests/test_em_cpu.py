"""kmcp-refstats --profile (cli/kmcp_refstats.cpp: stage 4/4 of `kmcp profile`) on crafted search results against our rule in Python
integers (tests/em_reference.py): the table must be equal BYTE FOR BYTE.

The samples are lists of reads (NumKmers, qLen, [(column, mKmers)]) over references of three chunks each (column = 3 * reference + chunk),
printed as search results.  Stage 3 — where the loop starts — is restated here in integers for what the samples need: every reference has
unique reads of its own in every chunk, so stage 1 keeps all of them (asserted on the tool's stage-1 output), and the tool runs with
--no-amb-corr, so stage 3 is the shares of recount_rule.hpp without the elimination.

Every case also runs against the literal float64 restatement of the reference's own expressions (tests/em_reference.py (b):
float_profile, started from tests/recount_reference.py's stage 3).  Ours differs from it only by the quantisation of the shares — at most
64 / EM_UNIT = 2.2e-8 read per split read and pass — and by the order floats are added in.  Compared exactly: the verdicts after pass 0,
the number of passes, whether the loop converged, the order of the lines.  The samples keep every threshold and the convergence test
away from a tie, and `against_b` asserts that margin on (b) itself.  Coverage and percentage are compared relatively: the largest
deviation over all cases of this file is RECORDED (also in DESIGN.md §4, K9) and BOUND = ten times that, capped at 1e-6, is asserted."""
import gzip
import os
import subprocess

import pytest

from tests import em_reference as E
from tests import filter_cases as FC
from tests import filter_reference as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "kmcp_amd", "kmcp-refstats")
UNIT, BASE = E.UNIT, E.BASE
TLEN = 30000
H = 0.75
LOOSE = dict(r=1, u=1, U=1, P=0.01, p=0.8, d=10.0, norm="mean")
TAXIDS = {"ref000": 111, "ref001": 112, "ref002": 121}  # ref000 and ref001 under species 110, ref002 under species 120
SPECIES = {0: 110, 1: 110, 2: 120}
RECORDED = 4.6e-10  # the largest deviation over the cases of this file (4.597e-10: the sample of several passes stopped by -I 1)
BOUND = min(10 * RECORDED, 1e-6)
SEEN = []  # the deviations of this run, printed by every case


def run(args, expect=0):
    if not os.path.exists(TOOL):
        import __graft_entry__ as g
        g.build()
    r = subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, timeout=120)
    assert r.returncode == expect, (r.returncode, r.stderr.decode())
    return r


def tsv_of(reads):
    out = []
    for i, (nk, ql, rows) in enumerate(reads):
        for c, n in rows:
            out.append("\t".join([f"q{i}", str(ql), str(nk), "1.0000e-03", "1", "ref%03d" % (c // 3), str(c % 3), "3", str(TLEN), "21", str(n), "%.4f" % (n / nk), "0.0100", "0.0100",
                                  str(i)]) + "\n")
    return "".join(out)


def unique_reads(ref, n, count=120, qlen=150):
    """n single-target reads of `ref`, a third on each chunk"""
    return [(130, qlen, [(3 * ref + i % 3, count)]) for i in range(n)]


def shared_reads(refs, n, count=110, qlen=150):
    """n reads that hit every reference of `refs` once, the chunk going round"""
    return [(130, qlen, [(3 * r + i % 3, count) for r in refs]) for i in range(n)]


def stage3(reads, n_cols, species, level_species, cut=None):
    """recount_rule.hpp without the elimination: [n_cols][4] in units (every reference is kept by stage 1: the cuts see all rows)"""
    cnt = [[0] * 4 for _ in range(n_cols)]
    target = [c // 3 for c in range(n_cols)]
    for nk, ql, all_rows in reads:
        rows = E.kept_rows(nk, all_rows, target, [1] * n_cols, cut)
        by = {}
        for i, (c, _) in enumerate(rows):
            by.setdefault(c // 3, []).append(i)
        ns = len(by)
        sp = {species[rows[ix[0]][0]] if species is not None else 0 for ix in by.values()}
        uniq_first = ns == 1 or (level_species and len(sp) == 1 and 0 not in sp)
        for t, ix in by.items():
            m = len(ix)
            for k, i in enumerate(ix):
                c, n = rows[i]
                share = UNIT - (m - 1) * (UNIT // m) if k == 0 else UNIT // m
                cnt[c][0] += share
                cnt[c][3] += ql * BASE // (ns * m)
                if k == 0 and uniq_first:
                    u = UNIT if ns == 1 else share
                    cnt[c][1] += u
                    if E.qcov(n, nk) >= H:
                        cnt[c][2] += u
    return cnt


def rollup3(w, tlen, th):
    """recount_rollup (recount_rule.hpp) -> (ok, coverage)"""
    n = len(w)
    match, uniq, hic, bases = (sum(x[j] for x in w) for j in range(4))
    covered = sum(1 for x in w if x[0] >= th["r"] * UNIT)
    frac = float(covered) / float(n)
    stdev, cov = 0.0, 0.0
    if bases:
        qlens = float(bases) / float(BASE)
        stdev = E.stdev([float(x[3]) / float(BASE) / qlens * float(n) for x in w])
        nz = [x[3] for x in w if x[3]]
        top = qlens if th["norm"] == "mean" else float(min(nz) if th["norm"] == "min" else max(nz)) / float(BASE) * float(n)
        cov = top / float(tlen)
    ok = match > 0 and not (uniq < th["u"] * UNIT or hic < th["U"] * UNIT or float(hic) < th["P"] * float(uniq) or frac < th["p"] or stdev > th["d"])
    return ok and cov > 0, cov


def expected(reads, n_refs, th, level_species=False, iters=10, pct=0.01, F=0.0, cut=None):
    """(a) -> (the table, the result of the loop, the names in table order)"""
    n_cols = 3 * n_refs
    target = [c // 3 for c in range(n_cols)]
    species = [SPECIES[c // 3] for c in range(n_cols)] if level_species else None
    s3 = stage3(reads, n_cols, species, level_species, cut)
    classes = [dict(columns=[3 * r, 3 * r + 1, 3 * r + 2], tlen=TLEN, name="ref%03d" % r) for r in range(n_refs)]
    start = [rollup3(s3[3 * r:3 * r + 3], TLEN, th) for r in range(n_refs)]

    def do_pass(est, cov):
        cols, tot = E.em_cols(reads, n_cols, target, species, est, cov, H, level_species, cut)
        return cols, tot["assigned_reads"]
    res = E.run(classes, [int(ok) for ok, _ in start], [c for _, c in start], th, do_pass, max_iters=iters, pct_threshold=pct)
    order = E.finish(classes, res, F)
    res["names"] = [classes[c]["name"] for c in order]
    res["by_name"] = {classes[c]["name"]: res["refs"][c] for c in order}
    res["verdicts0"] = {classes[c]["name"]: v for c, v in res["verdicts0"].items()}
    return E.table(classes, res, order), res


def against_b(text, res, th, level_species=False, tax=None, iters=10, pct=0.01, F=0.0, cut=None):
    """(a)'s result — the tool's, byte for byte — against the float restatement of the reference on the same search result"""
    kw = dict(level="species", taxid_map=tax[2], tax=tax[3]) if level_species else dict(level="strain")
    cut = cut or {}
    cuts = dict(max_fpr=1, min_qcov=0, top_n=cut.get("top_n", 0), keep_perfect=False, keep_main=cut.get("keep_main", False), max_gap=cut.get("max_gap", 0.4))
    start = E.float_start([text], th, H, no_amb_corr=True, **kw, **cuts)
    b = E.float_profile([text], start, th, hic_min_qcov=H, max_iters=iters, pct_threshold=pct, filter_low_pct=F, **kw, **cuts)
    # the sample is away from every tie, by far more than the two arithmetics can differ
    assert b["margin"] > 1e-4 and b["conv_margin"] > 1e-4 * min(1.0, 100 * pct), (b["margin"], b["conv_margin"])
    assert b["verdicts0"] == res["verdicts0"], (b["verdicts0"], res["verdicts0"])
    assert (b["passes"], b["converged"], b["order"], b["assigned"]) == (res["passes"], res["converged"], res["names"], res["assigned"])
    dev = 0.0
    for name in b["order"]:
        r = res["by_name"][name]
        for ours, theirs in ((r["coverage"], b["coverage"][name]), (r["percentage"], b["percentage"][name])):
            dev = max(dev, abs(ours - theirs) / abs(theirs))
        for ours, theirs in zip((r["match"], r["uniq"], r["hic"]), b["reads"][name]):
            assert abs(float(ours) / float(E.EM_UNIT) - theirs) <= 1e-6 * max(1.0, theirs)
    SEEN.append(dev)
    print(f"largest relative deviation of coverage / percentage from the float restatement: this case {dev:.3e}, this run {max(SEEN):.3e}")
    assert dev <= BOUND, (dev, BOUND)
    return b


def flags_of(th):
    return ["-f", "1", "-t", "0", "--no-amb-corr", "-H", H, "-r", th["r"], "-u", th["u"], "-U", th["U"], "-P", th["P"], "-p", th["p"], "-d", th["d"], "--norm-abund", th["norm"]]


def tool(tmp_path, reads, th, level_species=False, tax=None, iters=10, pct=0.01, F=0.0, cut=None):
    """the tool's table, equal to (a)'s byte for byte and held against (b); -> (the table, (a)'s result)"""
    text = tsv_of(reads)
    (tmp_path / "in.tsv").write_text(text)
    lv = ["--level", "species", "-T", tax[1], "-X", tax[0]] if level_species else ["--level", "strain"]
    extra = ["-I", iters, "--abund-pct-threshold", repr(pct), "-F", F]
    if cut:
        extra += (["-n", cut["top_n"]] if cut.get("top_n") else []) + (["--keep-main-matches", "--max-qcov-gap", cut["max_gap"]] if cut.get("keep_main") else [])
    run(flags_of(th) + lv + extra + ["-o", tmp_path / "s1.tsv", "--profile", tmp_path / "p.tsv", tmp_path / "in.tsv"])
    s1 = [l.split("\t") for l in (tmp_path / "s1.tsv").read_text().splitlines() if not l.startswith("#")]
    assert s1 and all(f[7] == "ok" for f in s1), "stage 1 must keep every reference of the sample"
    got = (tmp_path / "p.tsv").read_text()
    n_refs = max(c for _, _, rows in reads for c, _ in rows) // 3 + 1
    want, res = expected(reads, n_refs, th, level_species, iters, pct, F, cut)
    assert got == want
    against_b(text, res, th, level_species, tax, iters, pct, F, cut)
    return got, res


def head(text):
    lines = text.splitlines()
    return int(lines[0].split(": ")[1]), int(lines[1].split(": ")[1]), lines[2].split(": ")[1], [l.split("\t")[0] for l in lines[4:]]


@pytest.fixture(scope="module")
def tax(tmp_path_factory):
    d = tmp_path_factory.mktemp("taxdump")
    dump = FC.write_taxdump(d / "dump")
    FC.write_map(d / "map.tsv", TAXIDS)
    tmap = str(d / "map.tsv")
    return dump, tmap, FR.read_taxid_maps([tmap]), FR.Taxonomy(dump)


def skewed():
    """ref000 has twice the unique reads of ref001 and they share 60 reads; ref002 stands nearly alone: the loop moves the shared reads
    over and converges after nine passes"""
    return unique_reads(0, 60) + unique_reads(1, 30) + shared_reads([0, 1], 60) + unique_reads(2, 45) + shared_reads([0, 1, 2], 30)


def test_a_sample_that_needs_several_passes_and_one_stopped_by_I(tmp_path):
    got, res = tool(tmp_path, skewed(), LOOSE)
    assigned, passes, converged, names = head(got)
    assert assigned == len(skewed()) and 3 <= passes < 11 and converged == "yes" and names[0] == "ref000" and len(names) == 3
    got1, _ = tool(tmp_path, skewed(), LOOSE, iters=1)
    assert head(got1)[1:3] == (2, "no") and got1 != got
    # a threshold no pass gets under: all eleven passes
    got11, _ = tool(tmp_path, skewed(), LOOSE, pct=1e-13)
    assert head(got11)[1:3] == (11, "no")
    # .gz is honoured
    run(flags_of(LOOSE) + ["--level", "strain", "-o", tmp_path / "s1.tsv", "--profile", tmp_path / "p.tsv.gz", tmp_path / "in.tsv", "--abund-pct-threshold", "1e-13"])
    assert gzip.open(tmp_path / "p.tsv.gz", "rt").read() == got11


def test_unique_reads_alone_converge_at_pass_1(tmp_path):
    reads = unique_reads(0, 30) + unique_reads(1, 12) + unique_reads(2, 9, qlen=100)
    got, _ = tool(tmp_path, reads, LOOSE)
    assert head(got) == (51, 2, "yes", ["ref000", "ref001", "ref002"])


def dropped_samples():
    """at level species ref000 and ref001 are one species: stage 3 gives each HALF of a shared read's uniq, hic, match and bases, pass 0 gives
    ref001 its share by coverage — less than a quarter.  A threshold between the two lets ref001 pass stage 3 and fail after pass 0; from
    pass 1 on the 60 shared reads are unique reads of ref000.  One sample per test of profile.go:2372-2480, in its order"""
    base = unique_reads(0, 90) + shared_reads([0, 1], 60) + unique_reads(2, 33)  # (33: no count sits on a threshold of 30)
    low_qcov = [(130, 150, [(3 + i % 3, 90)]) for i in range(5)] + [(130, 150, [(3, 120)])]  # five unique reads below H, one above
    on_one_chunk = [(130, 150, [(3, 120)])] * 6
    return [("few-unique", base + unique_reads(1, 6), dict(LOOSE, u=30)),
            ("few-hic-unique", base + unique_reads(1, 6), dict(LOOSE, U=30)),
            ("low-hic-unique-prop", base + low_qcov, dict(LOOSE, P=0.8)),
            ("low-chunks-fraction", base + unique_reads(1, 6), dict(LOOSE, r=9, p=1.0)),
            ("high-depth-stdev", base + on_one_chunk, dict(LOOSE, d=0.3))]


@pytest.mark.parametrize("which", range(5), ids=[x[0] for x in dropped_samples()])
def test_a_reference_dropped_after_pass_0_leaves_its_reads_to_the_others(tmp_path, tax, which):
    verdict, reads, th = dropped_samples()[which]
    got, res = tool(tmp_path, reads, th, level_species=True, tax=tax)
    assert res["verdicts0"] == {"ref000": "ok", "ref001": verdict, "ref002": "ok"}
    assigned, passes, converged, names = head(got)
    assert names == ["ref000", "ref002"] and assigned == len(reads) - 6 and passes >= 2
    # the 60 shared reads ended as unique reads of ref000: 150 reads, all of them unique and above H
    assert got.splitlines()[4].split("\t")[6:9] == ["150", "150", "150"]


def test_one_species_against_two_and_strain_level(tmp_path, tax):
    """uniq of split reads only under one species"""
    mixed = unique_reads(0, 30) + unique_reads(1, 20) + unique_reads(2, 20) + shared_reads([0, 1], 40) + shared_reads([0, 2], 40)
    sp, _ = tool(tmp_path, mixed, LOOSE, level_species=True, tax=tax)
    st, _ = tool(tmp_path, mixed, LOOSE)
    ureads = lambda text: {l.split("\t")[0]: int(l.split("\t")[7]) for l in text.splitlines()[4:]}  # noqa: E731
    assert ureads(st) == {"ref000": 30, "ref001": 20, "ref002": 20} and ureads(sp)["ref001"] > 20 and ureads(sp)["ref002"] == 20


@pytest.mark.parametrize("norm", ["mean", "min", "max"])
def test_norm_abund(tmp_path, norm):
    reads = [(130, 150, [(0, 120)])] * 30 + [(130, 150, [(1, 120)])] * 20 + [(130, 150, [(2, 120)])] * 10 + unique_reads(1, 30) + shared_reads([0, 1], 50)
    th = dict(LOOSE, norm=norm)
    got, _ = tool(tmp_path, reads, th)
    if norm != "mean":
        assert got != expected(reads, 2, LOOSE)[0]


def test_filter_low_pct_and_ties_in_coverage(tmp_path):
    # ref001 and ref002 tie in coverage and chunksFrac: the name decides; ref003 is small
    reads = unique_reads(0, 90) + unique_reads(2, 30) + unique_reads(1, 30) + unique_reads(3, 6)
    plain, _ = tool(tmp_path, reads, LOOSE)
    assert head(plain)[3] == ["ref000", "ref001", "ref002", "ref003"]
    pct = [float(l.split("\t")[1]) for l in plain.splitlines()[4:]]
    assert pct[1] == pct[2] and 3 < pct[3] < 4
    for F, left in ((3, 4), (4, 3), (99.9, 1)):
        got, _ = tool(tmp_path, reads, LOOSE, F=F)
        assert len(head(got)[3]) == left, F
    assert got.splitlines()[4].split("\t")[1] == "100.000000"
    # one reference left: -F does not act
    tool(tmp_path, unique_reads(0, 30), LOOSE, F=99.9)


def test_row_cuts_with_a_row_outside_the_whitelist_between_kept_rows(tmp_path, tax):
    """a read hits ref000 (qCov 0.92), ref001 (0.50) and ref002.  --keep-main-matches --max-qcov-gap 0.4: while ref001 is on the whitelist
    the gap 0.92 - 0.50 cuts its row and everything after it.  Once ref001 has left (few-unique after pass 0) its row is skipped BEFORE
    the cut: with ref002 at 0.46 the gap 0.92 - 0.46 still cuts it, with ref002 at 0.55 it does not, and ref002 shares the nine reads.
    -n: with ref001 at ref000's qCov, -n 1 keeps both and cuts ref002 in every pass; -n 2 keeps all three.  Whole tables, byte for byte"""
    base = unique_reads(0, 90) + unique_reads(1, 6) + shared_reads([0, 1], 60) + unique_reads(2, 33)
    th = dict(LOOSE, u=30)
    main = dict(keep_main=True, max_gap=0.4)
    for third in (60, 72):
        reads = base + [(130, 150, [(0, 120), (3, 65), (6, third)])] * 9
        got, res = tool(tmp_path, reads, th, level_species=True, tax=tax, cut=main)
        rows = {l.split("\t")[0]: l.split("\t") for l in got.splitlines()[4:]}
        assert set(rows) == {"ref000", "ref002"} and res["verdicts0"]["ref001"] == "few-unique"
        assert (rows["ref002"][6] == "33") == (third == 60), rows["ref002"]
        assert head(got)[0] == len(reads) - 6
    reads = base + [(130, 150, [(0, 120), (3, 120), (6, 100)])] * 9
    one, _ = tool(tmp_path, reads, th, level_species=True, tax=tax, cut=dict(top_n=1))
    two, _ = tool(tmp_path, reads, th, level_species=True, tax=tax, cut=dict(top_n=2))
    none, _ = tool(tmp_path, reads, th, level_species=True, tax=tax)
    reads_of = lambda text: {l.split("\t")[0]: l.split("\t")[6] for l in text.splitlines()[4:]}  # noqa: E731
    assert reads_of(one)["ref002"] == "33" and reads_of(two)["ref002"] != "33" and two == none and one != two


def test_refusals(tmp_path):
    (tmp_path / "in.tsv").write_text(tsv_of(unique_reads(0, 3)))
    f = str(tmp_path / "in.tsv")
    p = str(tmp_path / "p.tsv")
    ok = ["--level", "strain"]
    for args, word in ((["--profile", p], "stdin"), (["--profile", p, "-"], "stdin"), (["--profile", f, f], "input file"), (["--profile", p, "-o", p, f], "out file"),
                       (["--profile", "-", f], "out file"), (["--profile", p, "--cooccur", p, f], "--cooccur"), (["--profile", p, "--recount", p, f], "--recount"),
                       (["--profile", p, "-m", "0", f], "-m 0"), (["--profile", p, "-I", "0", f], "abund-max-iters"), (["--profile", p, "--abund-pct-threshold", "0", f], "abund-pct-threshold"),
                       (["--profile", p, "-F", "100", f], "filter-low-pct"), (["--profile", p, "-F", "-1", f], "filter-low-pct")):
        r = run(ok + args, expect=255)
        assert word in r.stderr.decode(), (args, r.stderr.decode())
        assert not os.path.exists(p)
    # without the flag every output is what it is with it
    run(ok + ["-f", "1", "-t", "0", "-o", tmp_path / "a.tsv", "--cooccur", tmp_path / "ca.tsv", "--recount", tmp_path / "ra.tsv", f])
    run(ok + ["-f", "1", "-t", "0", "-o", tmp_path / "b.tsv", "--cooccur", tmp_path / "cb.tsv", "--recount", tmp_path / "rb.tsv", "--profile", p, f])
    for x in ("", "c", "r"):
        assert (tmp_path / f"{x}a.tsv").read_bytes() == (tmp_path / f"{x}b.tsv").read_bytes()
    assert os.path.exists(p)
