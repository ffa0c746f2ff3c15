"""Taxonomic binning end to end: K11 inside `kmcp-search --binning` and the library's bins route (kmcpg_submit_bins / kmcpg_wait_bins), on
the family database, reads and taxonomy B of tests/test_gpu_refstats.py (its fixture and helpers are imported, the file is not touched),
800 reads at -t 0.75 plus the fixture's long query above the device's -f bound.

The contract: `kmcp-search --ref-stats ... --ref-stats-profile P -o tsv`, then `kmcp-refstats -f 1 -t 0 ... --profile P2 --binning B1` on
that TSV (P2 is P), then `kmcp-search --binning B2 --binning-refs P`: B1 = B2 = the restatement of profile.go:2591-2784
(tests/binning_reference.py) over P's references, byte for byte.  Taxonomy B puts the strains of a base genome by turns into two species
of one genus, so the file holds strain, species, genus and higher TaxIds.  The configuration is that of tests/test_gpu_profile.py —
species level at mode 1 with --ref-stats-min-chunks-fraction 0 and R = 0.9: on the oracle's TSV of this sample through kmcp-refstats the EM
ends with 33 of the 51 references and the file holds 259 strain, 275 species, 87 genus and 27 higher TaxIds, 13 reads with matches get no
line, and the long query has one.  (Modes 2 to 5, mode 5 of the imported CONFIGS among them, end with NO reference on 800 reads: stage 3's
thresholds ask for more reads per chunk than the sample has.)  test_the_sample_is_not_vacuous asserts all five kinds."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import binning_reference as BR
from tests import filter_reference as FR
from tests import synth
from tests.binning_cases import lca_of, preorder
from tests.test_gpu_cli import CLI
from tests.test_gpu_recount import S_FLAGS, T_FLAGS
from tests.test_gpu_refstats import MIN_QCOV, TOOL, family, flags, run  # noqa: F401 (family: the fixture)

pytestmark = pytest.mark.gpu

CONFIG = ("B", "species", 1, None, 0.0)
EINVAL, EUNSUPPORTED = -1, -6
NONE = 0xFFFFFFFF
LINE = re.compile(r"^(\d+) reads searched, (\d+) binned; (\d+) reads \((\d+) pairs\) left to the host, (\d+) bytes from the device$", re.M)


def kinds(text):
    """the TaxIds of a binning file by their place in taxonomy B (tests/test_gpu_refstats.py write_taxdump)"""
    ids = [int(l.split("\t")[1]) for l in text.splitlines() if l[0] not in "#@"]
    return dict(strain=sum(t >= 50000 for t in ids), species=sum(1000 <= t < 50000 for t in ids), genus=sum(100 <= t < 1000 for t in ids), higher=sum(t < 100 for t in ids))


@pytest.fixture(scope="module")
def sample(family, tmp_path_factory):
    """the reads with the long query behind them as FASTQ (single, and as pairs with themselves), the plain search's TSV and profile P, and
    B1 = kmcp-refstats --binning of that TSV"""
    d = tmp_path_factory.mktemp("binning")
    reads = family["reads"] + [family["long_query"]]
    fq = str(d / "r.fq")
    with open(fq, "wb") as fh:
        for i, r in enumerate(reads):
            fh.write(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
    dump, tmap = family["tax"]["B"]
    s, t = flags(family, *CONFIG)
    out = {}
    for form, inputs in (("single", [fq]), ("paired", ["-1", fq, "-2", fq])):
        tsv, P = str(d / f"{form}.tsv"), str(d / f"{form}.P.tsv")
        run([CLI, "-d", family["root"], "-t", MIN_QCOV] + inputs + ["-o", tsv, "-q", "--ref-stats", d / "R.tsv", "--ref-stats-cooccur", d / "C.tsv", "--ref-stats-recount", d / "F.tsv",
                                                                   "--ref-stats-profile", P] + s + S_FLAGS)
        B1, P2 = str(d / f"{form}.tool.binning"), str(d / f"{form}.P2.tsv")
        run([TOOL] + t + T_FLAGS + ["-o", d / "s1.tsv", "--profile", P2, "--binning", B1, "--sample-id", "family", tsv])
        assert open(P2).read() == open(P).read()
        out[form] = dict(inputs=inputs, tsv=open(tsv).read(), P=P, B1=open(B1).read(), whitelist=BR.whitelist_of_profile(open(P).read()))
    return dict(d=d, fq=fq, reads=reads, dump=dump, tmap=tmap, tmap_ids=FR.read_taxid_maps([tmap]), taxo=FR.Taxonomy(dump), **out)


def test_the_sample_is_not_vacuous(sample):
    for form in ("single", "paired"):
        x = sample[form]
        k = kinds(x["B1"])
        queries = {l.split("\t")[0] for l in x["tsv"].splitlines() if l and l[0] != "#"}
        no_line = len(queries) - sum(k.values())
        print(f"{form}: {len(x['whitelist'])} references, bins {k}, {no_line} reads with matches and no line")
        assert min(k.values()) >= 1 and no_line >= 1, (form, k, no_line)
        assert x["B1"] == BR.binning([x["tsv"]], x["whitelist"], sample["tmap_ids"], sample["taxo"], sample_id="family", max_fpr=1, min_qcov=0)
    assert "r800\t" in sample["single"]["B1"], "the long query, binned by the host half, has a line"


def search_bins(family, sample, form, name, extra=(), env=None):
    x = sample[form]
    B2 = str(sample["d"] / f"{name}.binning")
    before = set(os.listdir(sample["d"]))
    r = run([CLI, "-d", family["root"], "-t", MIN_QCOV] + x["inputs"] + ["--binning", B2, "--binning-refs", x["P"], "--taxid-map", sample["tmap"], "--taxdump", sample["dump"],
                                                                      "--binning-sample-id", "family"] + list(extra), env=env)
    assert set(os.listdir(sample["d"])) - before == {f"{name}.binning"}, "the binning file and nothing else"
    m = LINE.search(r.stderr)
    assert m, r.stderr
    return open(B2).read(), [int(v) for v in m.groups()]


@pytest.mark.parametrize("form", ["single", "batches and threads", "paired", "every read to the host half"])
def test_cli_writes_the_file_kmcp_refstats_writes(family, sample, form):
    kind = "paired" if form == "paired" else "single"
    extra = ["-q", "-j", "4", "--gpu-batch", "300"] if form == "batches and threads" else [] if form == "single" else ["-q"]
    env = dict(os.environ, KMCPG_BIN_DEVICE="0") if form.startswith("every") else None
    got, (n, binned, host, left_pairs, nbytes) = search_bins(family, sample, kind, form.replace(" ", "_"), extra, env)
    assert got == sample[kind]["B1"], form
    lines = sum(1 for l in got.splitlines() if l[0] not in "#@")
    assert (n, binned) == (len(sample["reads"]), lines)
    batches = -(-n // 300) if form == "batches and threads" else 8  # (at most: the reader may cut a file into a few batches)
    if env:
        assert host == sum(1 for q in {l.split("\t")[0] for l in sample[kind]["tsv"].splitlines() if l and l[0] != "#"}) > 600, "every read with a match"
    else:
        assert 1 <= host < 20, "the long query is above the -f bound, the reads are not"
    assert 4 * n < nbytes <= 16 * n + 264 * batches + 8 * left_pairs


def test_gz_and_the_suffix_rule(family, sample):
    import gzip
    x = sample["single"]
    B = str(sample["d"] / "sfx")
    run([CLI, "-d", family["root"], "-t", MIN_QCOV, sample["fq"], "-q", "--binning", B, "--binning-refs", x["P"], "--taxid-map", sample["tmap"], "--taxdump", sample["dump"],
         "--binning-sample-id", "family"])
    assert not os.path.exists(B) and gzip.open(B + ".binning.gz", "rt").read() == x["B1"]


def plan_of(db, sample, whitelist):
    """the plan of bin_rule.hpp, built here in Python: (node_of_column, parent, last, taxid)"""
    n = int(db.info.n_cols)
    names = [db.col_info(c)[0] for c in range(n)]
    tree = {}
    for name in whitelist:
        line = sample["taxo"].lineage(sample["tmap_ids"][name])
        for a, b in zip(line, line[1:] + [0]):
            tree[a] = b
    parent, last, taxid, num = preorder(tree)
    wl = set(whitelist)
    node = np.array([num[sample["tmap_ids"][x]] if x in wl else NONE for x in names], dtype=np.uint32)
    return names, node, parent, last, taxid


def rule_on_pairs(res, names, sample, whitelist):
    """bin_rule.hpp's result from the pairs of a result, by the restatement's LCA fold"""
    wl = set(whitelist)
    out = np.full(len(res.offs) - 1, NONE, dtype=np.uint32)
    for r in range(len(out)):
        ids = sorted({sample["tmap_ids"][names[int(c)]] for c in res.pairs[int(res.offs[r]):int(res.offs[r + 1]), 0] if names[int(c)] in wl})
        if ids:
            t = ids[0]
            for t2 in ids[1:]:
                t = BR.lca(sample["taxo"], t, t2)
            out[r] = t
    return out


@pytest.mark.parametrize("form", ["one ticket", "tickets in flight", "paired", "every read to the host half"])
def test_library_bins_equal_the_rule_on_the_pairs(family, sample, form, monkeypatch):
    from kmcp_amd import Database, default_params, lib
    if form.startswith("every"):
        monkeypatch.setenv("KMCPG_BIN_DEVICE", "0")
    reads = sample["reads"]
    mates = reads if form == "paired" else None
    p = default_params(min_qcov=MIN_QCOV)
    whitelist = sample["paired" if mates else "single"]["whitelist"]
    with Database.open(family["db_dir"], device=0) as db:
        names, node, parent, last, taxid = plan_of(db, sample, whitelist)
        pairs = db.search_pairs(reads, mates, params=p)
        want = rule_on_pairs(pairs, names, sample, whitelist)
        assert (want != NONE).sum() > 300 and (want == NONE).sum() > 0
        db.set_binning(node, parent, last, taxid)
        if form == "tickets in flight":
            cuts = [0, 300, 600, len(reads)]
            tickets = [db.submit_bins(*lib.pack_reads(reads[a:b]), params=p) for a, b in zip(cuts, cuts[1:])]
            parts = [db.wait_bins(t) for t in tickets]
            got = np.concatenate([b for b, _ in parts])
            st = {k: sum(s[k] for _, s in parts) for k in parts[0][1]}
            n_tickets = 3
        else:
            got, st = db.search_bins(reads, mates, params=p)
            n_tickets = 1
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, f"{form}: read {bad[0]} has bin {got[bad[0]]}, the rule says {want[bad[0]]}; {len(bad)} differ"
        n = len(reads)
        assert st["n_reads"] == n and st["binned_reads"] == int((want != NONE).sum()) and st["kept_pairs"] == len(pairs.pairs)
        assert st["host_reads"] >= 1, "the long query is above the device's -f bound"
        if form.startswith("every"):
            assert st["host_reads"] == int((np.diff(pairs.offs.astype(np.int64)) > 0).sum()) and st["left_pairs"] == st["kept_pairs"]
        else:
            assert st["host_reads"] < 20
        assert 4 * n < st["bytes_d2h"] <= 16 * n + 264 * n_tickets + 8 * st["left_pairs"]
        assert st["reruns"] == 0, "the family sample cannot overflow a hit buffer (test_a_batch_that_is_run_again_is_binned_by_its_rerun has one that does)"
        w, _ = db.last_bins()
        assert w["bad_segments"] == 0 and w["skipped"] == 0 and w["left"] == (st["host_reads"] if n_tickets == 1 else w["left"]) and w["in_lds"] == 1
        # a batch without a LEFT read: the bins, the counters and the witnesses, nothing else
        short = reads[:200]
        got2, st2 = db.search_bins(short, short if mates else None, params=p)
        if not form.startswith("every"):
            assert st2["host_reads"] == 0 and st2["left_pairs"] == 0 and st2["bytes_d2h"] <= 4 * 200 + 256
        assert np.array_equal(got2, want[:200])
        db.set_binning()
        assert np.array_equal(db.search_pairs(reads, mates, params=p).pairs, pairs.pairs), "the search itself is what it was"


def test_a_batch_that_is_run_again_is_binned_by_its_rerun(tmp_path, monkeypatch):
    """The sample of tests/test_gpu_refstats.py test_a_batch_that_is_run_again_is_counted_once: 40 close relatives, every read matches ~35
    columns — more hits than the 8 n + 1024 a fresh lane has room for, and KMCPG_HIT_BUDGET_MB=0 keeps the buffers from growing ahead.  The
    first attempt of every bins ticket overflows: K11 and K10 see the hit counter above capacity and write nothing, kmcpg_wait_bins runs the
    batch again into a larger buffer, and the bins are the rerun's.  The witness is kmcpg_result_bins.reruns.  The relatives are leaves
    under four species of two genera; every other one is whitelisted."""
    from kmcp_amd import Database, default_params, lib
    monkeypatch.setenv("KMCPG_HIT_BUDGET_MB", "0")
    rng = np.random.default_rng(91)
    base = synth.random_genomes(1, 6000, seed=90)[0]
    genomes = []
    for i in range(40):
        g = np.frombuffer(base, dtype=np.uint8).copy()
        m = rng.random(len(g)) < 0.004
        g[m] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(m.sum()))
        genomes.append(g.tobytes())
    db_dir = synth.make_db(tmp_path / "db", genomes, k=21, n_chunks=2, overlap=150, threads=1)
    reads = synth.sample_reads([base], 1500, 150, sub_rate=0.0, seed=200, frac_random=0.1)
    p = default_params()
    n = len(reads)

    def plan(db):
        n_cols = int(db.info.n_cols)
        names = [db.col_info(c)[0] for c in range(n_cols)]
        refs = sorted(set(names))
        assert len(refs) == 40
        tree = {1: 0, 10: 1, 11: 1, 100: 10, 101: 10, 102: 11, 103: 11}
        taxid_of = {}
        for i, r in enumerate(refs):
            taxid_of[r] = 1000 + i
            tree[1000 + i] = 100 + i % 4
        whitelist = set(refs[::2])
        parent, last, taxid, num = preorder({t: q for t, q in tree.items() if t < 1000 or t in {taxid_of[r] for r in whitelist}})
        node = np.array([num[taxid_of[x]] if x in whitelist else NONE for x in names], dtype=np.uint32)
        return names, taxid_of, whitelist, tree, (node, parent, last, taxid)

    with Database.open(db_dir, device=0) as db:
        names, taxid_of, whitelist, tree, tables = plan(db)
        # the bins ticket FIRST, on a fresh lane (a lane keeps the buffer a rerun gave it); the pairs it is held against afterwards
        db.set_binning(*tables)
        got, st = db.search_bins(reads, params=p)
        assert st["reruns"] == 1, st
        w, _ = db.last_bins()
        assert w["skipped"] == 0 and w["bad_segments"] == 0 and w["several"] > 1000, "the witness is the rerun's: the attempt that overflowed was skipped and is not reported"
        pairs = db.search_pairs(reads, params=p)
        assert len(pairs.pairs) > 8 * n + 1024, "more matches than the first attempt's hit buffer holds"
        want = np.full(n, NONE, dtype=np.uint32)
        for r in range(n):
            ids = sorted({taxid_of[names[int(c)]] for c in pairs.pairs[int(pairs.offs[r]):int(pairs.offs[r + 1]), 0] if names[int(c)] in whitelist})
            if ids:
                want[r] = lca_of(ids, tree)
        assert (want != NONE).sum() > 1000 and (want == NONE).sum() > 50
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, f"read {bad[0]} has bin {got[bad[0]]}, the rule says {want[bad[0]]}; {len(bad)} differ"
        assert st["kept_pairs"] == len(pairs.pairs) and st["binned_reads"] == int((want != NONE).sum()) and st["host_reads"] == 0
        assert st["bytes_d2h"] <= 4 * n + 256, "the last attempt's bytes"
    with Database.open(db_dir, device=0) as db:  # two tickets in flight on two fresh lanes, each of them overflowing
        db.set_binning(*plan(db)[4])
        cuts = [0, 700, n]
        tickets = [db.submit_bins(*lib.pack_reads(reads[a:b]), params=p) for a, b in zip(cuts, cuts[1:])]
        parts = [db.wait_bins(t) for t in tickets]
        assert [s["reruns"] for _, s in parts] == [1, 1] and np.array_equal(np.concatenate([b for b, _ in parts]), want)


def test_ticket_refusals(family, sample):
    from kmcp_amd import Database, default_params, lib
    reads = sample["reads"][:64]
    p = default_params(min_qcov=MIN_QCOV)
    s, o = lib.pack_reads(reads)
    with Database.open(family["db_dir"], device=0) as db:
        names, node, parent, last, taxid = plan_of(db, sample, sample["single"]["whitelist"])
        with pytest.raises(lib.KmcpGpuError, match="kmcpg_set_binning") as e:
            db.submit_bins(s, o, params=p)
        assert e.value.code == EINVAL
        db.set_binning(node, parent, last, taxid)
        t = db.submit_bins(s, o, params=p)
        for wrong in (db.wait, db.wait_pairs, db.wait_summaries, db.wait_stats):
            with pytest.raises(lib.KmcpGpuError) as e:
                wrong(t)
            assert e.value.code == EINVAL and ("kmcpg_wait_bins" in str(e.value) or "not one of kmcpg_submit_stats" in str(e.value))
        bins, st = db.wait_bins(t)  # the ticket stayed valid
        assert st["n_reads"] == 64 and len(bins) == 64 and st["bytes_d2h"] <= 4 * 64 + 256
        t = db.submit(s, o, params=p)
        with pytest.raises(lib.KmcpGpuError, match="not one of kmcpg_submit_bins") as e:
            db.wait_bins(t)
        assert e.value.code == EINVAL
        db.wait_pairs(t)
        db.set_specific(np.arange(len(node), dtype=np.uint32), None)
        with pytest.raises(lib.KmcpGpuError, match="kmcpg_set_specific") as e:
            db.submit_bins(s, o, params=p)
        assert e.value.code == EINVAL
        db.set_specific()
        for kw in (dict(try_se=1), dict(top_n_scores=1)):
            with pytest.raises(lib.KmcpGpuError, match="kmcpg_set_binning") as e:
                db.submit_bins(s, o, params=default_params(**kw))
            assert e.value.code == EUNSUPPORTED


def test_cli_refuses_what_the_list_cannot_give(family, sample, tmp_path):
    """a listed name the database does not have, and a listed reference without a TaxId: refused before a batch is searched, nothing written"""
    x = sample["single"]
    listed = tmp_path / "list.tsv"
    listed.write_text("#ref\n" + x["whitelist"][0] + "\tsomething\nno-such-reference\n")
    base = [CLI, "-d", family["root"], "-t", str(MIN_QCOV), sample["fq"], "-q", "--binning", str(tmp_path / "b.binning")]
    r = subprocess.run(base + ["--binning-refs", str(listed), "--taxid-map", sample["tmap"], "--taxdump", sample["dump"]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "no reference no-such-reference" in r.stderr and sorted(os.listdir(tmp_path)) == ["list.tsv"], r.stderr
    short = tmp_path / "short.tsv"
    first = sorted(x["whitelist"])[0]
    short.write_text("".join(l for l in open(sample["tmap"]) if not l.startswith(first + "\t")))
    r = subprocess.run(base + ["--binning-refs", x["P"], "--taxid-map", str(short), "--taxdump", sample["dump"]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and f"unknown taxid for {first}" in r.stderr and sorted(os.listdir(tmp_path)) == ["list.tsv", "short.tsv"], r.stderr
