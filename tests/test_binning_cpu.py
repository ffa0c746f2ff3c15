"""kmcp-refstats --binning (cli/kmcp_refstats.cpp: the binning pass of `kmcp profile -B`) on crafted search results against the literal
restatement of profile.go:2591-2784 (tests/binning_reference.py): the file must be equal BYTE FOR BYTE; and the refusals of both command
lines — kmcp-search's before a file or a GPU is touched, as tests/test_search_stats_only_cpu.py checks them.

The references have three chunks each and unique reads of their own in every chunk, so that stages 1-4 keep them under LOOSE thresholds
(asserted on the profile); `dropped` has one read on one chunk and fails stage 1.  Their TaxIds in the crafted taxonomy of
tests/filter_cases.py: two strains of one species (111, 112), a strain of the genus' other species (121), the first species itself (110: an
ANCESTOR of 111), another family (410), a merged TaxId (999 -> 111) and one no file knows (777)."""
import gzip
import os
import subprocess

import pytest

from tests import binning_reference as BR
from tests import filter_cases as FC
from tests import filter_reference as FR
from tests.test_em_cpu import LOOSE, TOOL, flags_of, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kmcp_amd", "kmcp-search")
TAXIDS = {"ref000": 111, "ref001": 112, "ref002": 121, "ref003": 110, "ref004": 410, "ref005": 999, "ref006": 777, "dropped": 112}
KEPT = ["ref000", "ref001", "ref002", "ref003", "ref004", "ref005", "ref006"]
NK, TLEN = 130, 30000


def rows_of(query, rows):
    """rows: (reference, chunk, matched k-mers) -> the lines of one query"""
    return "".join("\t".join([query, "150", str(NK), "1.0000e-03", "1", ref, str(chunk), "3", str(TLEN), "21", str(n), "%.4f" % (n / NK), "0.0100", "0.0100", "0"]) + "\n"
                   for ref, chunk, n in rows)


def sample():
    """(the search result, what each named read is there for)"""
    out = []
    for r, ref in enumerate(KEPT):  # 12 unique reads per reference, four on each chunk: stages 1-4 keep all seven
        for i in range(12):
            out.append(rows_of(f"u{r}_{i}", [(ref, i % 3, 120)]))
    out.append(rows_of("only_dropped", [("dropped", 0, 125)]))  # the one read of `dropped`: stage 1 drops it for its chunks — and this read gets no line
    cases = {
        "siblings": [("ref000", 0, 120), ("ref001", 1, 118)],                        # 111, 112 -> species 110
        "one_target_three_rows": [("ref002", 0, 120), ("ref002", 1, 119), ("ref002", 2, 118)],
        "ancestor_with_descendant": [("ref003", 0, 120), ("ref000", 0, 119)],        # 110 and 111 -> 110
        "genus": [("ref000", 0, 120), ("ref002", 0, 119)],                           # 111, 121 -> genus 100
        "other_family": [("ref001", 0, 120), ("ref004", 0, 119)],                    # 112, 410 -> order 30
        "merged_alone": [("ref005", 2, 120)],                                        # 999 prints resolved: 111
        "merged_with_its_target": [("ref005", 0, 120), ("ref000", 1, 120)],          # one node: 111
        "unknown_alone": [("ref006", 1, 120)],                                       # 777 as it is mapped
        "unknown_beside": [("ref006", 0, 120), ("ref000", 0, 119)],                  # 0
        # the skip changes which row is first: `dropped` leads with a perfect row; with --keep-perfect-matches the first WHITELISTED row
        # (qCov < 1) opens the query and the rest is kept — were the perfect row the first, everything behind it would be cut
        "dropped_leads_perfect": [("dropped", 0, 130), ("ref000", 0, 125), ("ref002", 0, 124)],
        "dropped_between": [("ref001", 0, 126), ("dropped", 0, 125), ("ref001", 1, 120)],
        # the cuts: a perfect first row; a gap above 0.2 after the second row; three distinct scores
        "perfect_then_less": [("ref001", 0, 130), ("ref002", 0, 129)],               # --keep-perfect-matches: 112, else genus 100
        "gap": [("ref000", 0, 128), ("ref001", 0, 126), ("ref004", 0, 90), ("ref002", 0, 89)],  # --keep-main-matches --max-qcov-gap 0.2: 110, else 30
        "three_scores": [("ref000", 0, 128), ("ref000", 1, 128), ("ref001", 0, 120), ("ref004", 0, 110)],  # -n 1: 111; -n 2: 110; else 30
    }
    for q, rows in cases.items():
        out.append(rows_of(q, rows))
    return "".join(out), cases


@pytest.fixture(scope="module")
def tax(tmp_path_factory):
    d = tmp_path_factory.mktemp("bin_taxdump")
    dump = FC.write_taxdump(d / "dump")
    tmap = FC.write_map(d / "map.tsv", TAXIDS)
    return dump, tmap, FR.read_taxid_maps([tmap]), FR.Taxonomy(dump)


def bins_of(text):
    return dict(l.split("\t") for l in text.splitlines() if l and l[0] not in "#@")


def tool(tmp_path, tax, text, extra=(), binning="b.binning", want_whitelist=KEPT, sample_id=None, **cuts):
    """kmcp-refstats ... --profile P --binning B on `text`; B must equal the restatement over P's references, byte for byte -> B's text"""
    (tmp_path / "in.tsv").write_text(text)
    sid = ["--sample-id", sample_id] if sample_id is not None else []
    run(flags_of(LOOSE) + ["--level", "strain", "-T", tax[1], "-X", tax[0], "-o", tmp_path / "s1.tsv", "--profile", tmp_path / "p.tsv", "--binning", tmp_path / binning] + sid +
        list(extra) + [tmp_path / "in.tsv"])
    whitelist = BR.whitelist_of_profile((tmp_path / "p.tsv").read_text())
    assert sorted(whitelist) == sorted(want_whitelist)
    path = tmp_path / BR.file_name(binning)
    data = path.read_bytes()
    got = gzip.decompress(data).decode() if str(path).endswith(".gz") else data.decode()
    want = BR.binning([text], whitelist, tax[2], tax[3], sample_id=sample_id or "", max_fpr=1, min_qcov=0, **cuts)
    assert got == want
    return got


def test_the_rule_on_every_crafted_read(tmp_path, tax):
    text, cases = sample()
    got = tool(tmp_path, tax, text)
    assert got.startswith(BR.HEADER.format(""))
    b = bins_of(got)
    assert b["siblings"] == "110" and b["one_target_three_rows"] == "121" and b["ancestor_with_descendant"] == "110" and b["genus"] == "100"
    assert b["other_family"] == "30" and b["merged_alone"] == "111" and b["merged_with_its_target"] == "111"
    assert b["unknown_alone"] == "777" and b["unknown_beside"] == "0"
    assert b["dropped_leads_perfect"] == "100" and b["dropped_between"] == "112"
    assert b["perfect_then_less"] == "100" and b["gap"] == "30" and b["three_scores"] == "30"
    # a read whose only rows are of a dropped reference has matches and no line; every other read has one, in the order of the input
    assert "only_dropped" not in b and "only_dropped\t" in text
    queries = list(dict.fromkeys(l.split("\t")[0] for l in text.splitlines()))
    assert list(b) == [q for q in queries if q != "only_dropped"]


def test_each_cut_on_and_off(tmp_path, tax):
    text, _ = sample()
    plain = bins_of(tool(tmp_path, tax, text))
    perfect = bins_of(tool(tmp_path, tax, text, ["--keep-perfect-matches"], keep_perfect=True))
    # the whitelist skip comes first: `dropped`'s perfect row is no first row, so the two whitelisted rows behind it are both kept
    assert perfect["dropped_leads_perfect"] == "100" and perfect["perfect_then_less"] == "112" and plain["perfect_then_less"] == "100"
    main = bins_of(tool(tmp_path, tax, text, ["--keep-main-matches", "--max-qcov-gap", "0.2"], keep_main=True, max_gap=0.2))
    assert main["gap"] == "110" and plain["gap"] == "30"
    top1 = bins_of(tool(tmp_path, tax, text, ["-n", "1"], top_n=1))
    top2 = bins_of(tool(tmp_path, tax, text, ["-n", "2"], top_n=2))
    assert (top1["three_scores"], top2["three_scores"], plain["three_scores"]) == ("111", "110", "30")
    for other in (perfect, main, top1, top2):
        assert other != plain and set(other) == set(plain)


def test_suffix_rule_gz_and_the_sample_id(tmp_path, tax):
    text, _ = sample()
    plain = tool(tmp_path, tax, text, sample_id="S 1")
    assert plain.splitlines()[3] == "@SampleID:S 1" and plain.splitlines()[4] == "@@SEQUENCEID\tTAXID"
    # a name that ends in neither .binning nor .binning.gz gets .binning.gz; .binning.gz is honoured as it is
    assert tool(tmp_path, tax, text, binning="x.tsv", sample_id="S 1") == plain and (tmp_path / "x.tsv.binning.gz").exists() and not (tmp_path / "x.tsv").exists()
    assert tool(tmp_path, tax, text, binning="y.binning.gz", sample_id="S 1") == plain and not (tmp_path / "y.binning.gz.binning.gz").exists()
    assert tool(tmp_path, tax, text, binning="z.gz", sample_id="S 1") == plain and (tmp_path / "z.gz.binning.gz").exists()


def test_refusals_of_kmcp_refstats(tmp_path, tax):
    text, _ = sample()
    f = tmp_path / "in.tsv"
    f.write_text(text)
    base = flags_of(LOOSE) + ["--level", "strain", "-o", tmp_path / "s1.tsv"]
    tx = ["-T", tax[1], "-X", tax[0]]
    P, B = tmp_path / "p.tsv", tmp_path / "b.binning"
    for args, word in ((tx + ["--binning", B, f], "--profile is needed"), (["--profile", P, "--binning", B, f], "-T/--taxid-map and -X/--taxdump"),
                       (tx + ["--profile", P, "--binning", B], "stdin"), (tx + ["--profile", P, "--binning", B, "-"], "stdin"),
                       (tx + ["--profile", P, "--binning", tmp_path / "s1.tsv.binning", "-o", tmp_path / "s1.tsv.binning", f], "other out files"),
                       (tx + ["--profile", tmp_path / "q.binning", "--binning", tmp_path / "q.binning", f], "other out files")):
        r = run(base[:-2] + list(args) if "-o" in args else base + list(args), expect=255)
        assert word in r.stderr.decode(), (args, r.stderr.decode())
        assert not B.exists() and not P.exists()
    # an input file that is the binning file itself
    g = tmp_path / "g.binning"
    g.write_text(text)
    r = run(base + tx + ["--profile", P, "--binning", g, g], expect=255)
    assert "input file" in r.stderr.decode() and g.read_text() == text
    # a whitelisted reference without a TaxId: refused, the message names the first such reference, nothing is written
    short = tmp_path / "short.tsv"
    short.write_text("".join(f"{k}\t{v}\n" for k, v in TAXIDS.items() if k not in ("ref002", "ref004")))
    r = run(base + ["-T", short, "-X", tax[0], "--profile", P, "--binning", B, f], expect=255)
    assert "unknown taxid for ref002" in r.stderr.decode() and not B.exists() and not (tmp_path / "s1.tsv").exists()


def search(tmp_path, args):
    if not os.path.exists(CLI):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # a GPU, were it asked for, would not be there
    return subprocess.run([CLI, "-d", str(tmp_path / "no-such-db"), str(tmp_path / "no-such-reads.fq")] + [str(a) for a in args], capture_output=True, text=True, timeout=60, env=env)


def search_refused(tmp_path, args, *words):
    r = search(tmp_path, args)
    assert r.returncode == 255, (r.returncode, r.stderr)
    last = r.stderr.strip().splitlines()[-1]
    for w in words:
        assert w in last, (w, r.stderr)
    assert "no-such" not in r.stderr, r.stderr  # neither the database nor the input nor the list was looked at
    assert r.stdout == "" and os.listdir(tmp_path) == [], os.listdir(tmp_path)


def test_refusals_of_kmcp_search(tmp_path):
    B, L, M, X = tmp_path / "b.binning", tmp_path / "no-such-list.tsv", tmp_path / "no-such-map.tsv", tmp_path / "no-such-dump"
    on = ["--binning", B, "--binning-refs", L, "--taxid-map", M, "--taxdump", X]
    search_refused(tmp_path, on + ["-o", tmp_path / "out.tsv"], "-o/--out-file", "--binning", "no search result is written")
    search_refused(tmp_path, ["--binning", B, "--taxid-map", M, "--taxdump", X], "--binning needs --binning-refs")
    search_refused(tmp_path, ["--binning", B, "--binning-refs", L], "--taxid-map", "--taxdump", "--binning")
    search_refused(tmp_path, ["--binning", B, "--binning-refs", L, "--taxid-map", M], "--taxdump", "--binning")
    search_refused(tmp_path, ["--binning-refs", L], "--binning-refs", "only used with --binning")
    search_refused(tmp_path, ["--binning-sample-id", "S"], "--binning-sample-id", "only used with --binning")
    for stats in (["--ref-stats", tmp_path / "r.tsv"], ["--ref-stats", tmp_path / "r.tsv", "--ref-stats-only"], ["--ref-stats-mode", "5"], ["--ref-stats-only"],
                  ["--ref-stats-profile", tmp_path / "p.tsv"], ["--ref-stats-no-amb-corr"], ["--ref-stats-filter-low-pct", "1"], ["--ref-stats-cooccur", tmp_path / "c.tsv"]):
        search_refused(tmp_path, on + stats, "--ref-stats", "cannot be combined with --binning")
    # everything --ref-stats-only refuses
    for extra, word in ((["--specific-level", "strain"], "--specific-level"), (["--regions-bed", tmp_path / "r.bed"], "--regions-bed"), (["--also-db", tmp_path / "other"], "--also-db"),
                        (["-g"], "-g/--query-whole-file"), (["-K"], "-K/--keep-unmatched"), (["--try-se"], "--try-se"), (["-n", "2"], "-n/--keep-top-scores"),
                        (["--sliding-step", "100", "--sliding-window", "300"], "--sliding-"), (["--gpus", "2"], "--gpus/--gpu-ids"), (["--gpu-passes", "2"], "--gpu-passes")):
        search_refused(tmp_path, on + extra, word, "--binning")
    # the accepted form gets as far as the input, and still nothing is created
    r = search(tmp_path, on)
    assert r.returncode == 255 and "no-such" in r.stderr and os.listdir(tmp_path) == [], (r.stderr, os.listdir(tmp_path))
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "--binning-refs" in r.stdout + r.stderr


def test_kmcp_search_refuses_what_the_list_cannot_give_without_a_gpu(tmp_path, tax):
    """a listed name the database does not have, and a listed reference without a TaxId: the names come from a metadata-only handle, so both
    are refused before the GPU is touched (there is none here: had the command gone on, it would have said so) and nothing is written"""
    db, fq = os.path.join(ROOT, "shim", "testdata", "db"), os.path.join(ROOT, "shim", "testdata", "reads.fq")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = tmp_path / "out"
    out.mkdir()
    tmap = tmp_path / "map.tsv"
    tmap.write_text("g00000\t111\ng00001\t112\ng00003\t121\n")

    def refused(listed, word):
        lst = tmp_path / "list.tsv"
        lst.write_text(listed)
        r = subprocess.run([CLI, "-d", db, fq, "-q", "--binning", str(out / "b.binning"), "--binning-refs", str(lst), "--taxid-map", str(tmap), "--taxdump", tax[0]],
                           capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 255 and word in r.stderr.strip().splitlines()[-1], r.stderr
        assert "HIP" not in r.stderr and "device" not in r.stderr and os.listdir(out) == [], (r.stderr, os.listdir(out))

    refused("#ref\tpercentage\ng00001\t60\nno-such-reference\t40\n", "the database has no reference no-such-reference")
    refused("g00003\ng00002\ng00000\ng00004\n", "unknown taxid for g00002")  # the first in byte order
