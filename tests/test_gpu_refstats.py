"""Reference statistics end to end: K6 behind K3 inside the library's pipelines (kmcpg_set_refstats) and `kmcp-search --ref-stats`, on
the reduced real-genome family database (tools/family_db.py: 16 base genomes, 6 + 15 x 3 strains, 10 chunks each) under two
taxonomies the test writes:
  A  one species per base genome, its strains as children;
  B  the strains of each base genome alternately in two species of one genus.
Three things must agree: the file of `kmcp-search --ref-stats`, what `kmcp-refstats -f 1 -t 0` makes of the same run's TSV, and the plain
restatement of profile.go (tests/refstats_reference.py) on that TSV.  For the library the restatement runs on rows written from the
result's own records.

The searches run with -t 0.75 (as the species-specific tests do: at 0.55 nearly every read of this database matches every strain of its
base genome) on the first 800 of the sample's 3000 reads: with all of them every chunk of every reference has rows and nearly every
reference has a unique read, so stage 1 would say "ok" 50 times out of 51.  From the oracle's TSV of the 800 reads (51 references):
    taxonomy, level, mode     ok   no-unique   no-hic-unique   low-chunks-fraction
    B  species  5             24    6           7              14
    A  species  5             33    0           0              18
    -  strain   3, H = 0.9    15   14          22               0
CONFIGS are these three; test_the_sample_is_not_one_sided asserts the table's shape on the oracle's TSV."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import filter_reference as FR
from tests import refstats_reference as RR
from tests import synth
from tests.test_gpu_cli import CLI, HEADER, oracle_tsv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
TOOL = os.path.join(ROOT, "kmcp_amd", "kmcp-refstats")
MIN_QCOV = 0.75
VERDICTS = {"ok", "no-unique", "no-hic-unique", "low-chunks-fraction"}
N_SAMPLE = 800
# (taxonomy, level, mode, H or None, p or None).  Mode 3 at -t 0.75 cannot say no-hic-unique by itself (its H is 0.75); mode 5 (H 0.8, p 1) can
CONFIGS = [("B", "species", 5, None, None), ("A", "species", 5, None, None), (None, "strain", 3, 0.9, None)]


def write_taxdump(d, names, split):
    """nodes.dmp + a TaxId map for targets named ACCESSION.sNNNN: a genus per accession, its strains under one species or, `split`, by
    turns under two"""
    os.makedirs(d, exist_ok=True)
    accs = sorted({n.rsplit(".s", 1)[0] for n in names})
    lines, tmap = ["1\t|\t1\t|\tno rank\t|\t\t|\n", "2\t|\t1\t|\tsuperkingdom\t|\t\t|\n"], []
    for gi, acc in enumerate(accs):
        lines.append(f"{100 + gi}\t|\t2\t|\tgenus\t|\t\t|\n")
        for half in range(2 if split else 1):
            lines.append(f"{1000 + 2 * gi + half}\t|\t{100 + gi}\t|\tspecies\t|\t\t|\n")
    for n in sorted(set(names)):
        acc, s = n.rsplit(".s", 1)
        gi, si = accs.index(acc), int(s)
        lines.append(f"{50000 + 100 * gi + si}\t|\t{1000 + 2 * gi + (si % 2 if split else 0)}\t|\tstrain\t|\t\t|\n")
        tmap.append(f"{n}\t{50000 + 100 * gi + si}\n")
    open(os.path.join(d, "nodes.dmp"), "w").writelines(lines)
    open(os.path.join(d, "map.tsv"), "w").writelines(tmap)
    return str(d), os.path.join(d, "map.tsv")


@pytest.fixture(scope="module")
def family(oracle_lib, tmp_path_factory):
    import family_db
    from kmcp_amd import lib
    O = oracle_lib
    tmp = tmp_path_factory.mktemp("refstats")
    cols, reads, info = family_db.generate(ecoli_strains=6, small_strains=3, n_reads=3000)
    whole = lib.build_db(str(tmp / "db"), cols, k=family_db.K, threads=8, alias="family-db")
    names = [c[0] for c in cols]
    reads = reads[:N_SAMPLE]
    rl = [reads[i].tobytes() for i in range(reads.shape[0])]
    fq = str(tmp / "r.fq")
    family_db.write_fastq(fq, reads)
    tax = {"A": write_taxdump(str(tmp / "taxA"), names, False), "B": write_taxdump(str(tmp / "taxB"), names, True)}
    odb = O.OracleDB(whole)
    try:
        rows, _ = oracle_tsv(O, odb, [f"r{i}" for i in range(len(rl))], rl, params=O.default_params(min_qcov=MIN_QCOV))
    finally:
        odb.close()
    return dict(tmp=tmp, db_dir=whole, root=os.path.dirname(whole), reads=rl, fq=fq, tax=tax, oracle_rows=rows,
                long_query=family_db.base_genomes()[1][1][:3000])


def run(cmd, env=None):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    return r


def restated(family, text, tag, level, mode, H, p):
    kw = {}
    if tag:
        dump, tmap = family["tax"][tag]
        kw = dict(taxid_map=FR.read_taxid_maps([tmap]), tax=FR.Taxonomy(dump))
    return RR.refstats([text], mode=mode, min_hic_ureads_qcov=H, min_chunks_fraction=p, max_fpr=1, min_qcov=0, level=level, **kw)


def flags(family, tag, level, mode, H, p):
    """(kmcp-search's flags, kmcp-refstats' flags) of one configuration"""
    s, t = ["--ref-stats-mode", mode, "--ref-stats-level", level], ["-f", "1", "-t", "0", "-m", mode, "--level", level]
    if tag:
        dump, tmap = family["tax"][tag]
        s += ["--taxid-map", tmap, "--taxdump", dump]
        t += ["-T", tmap, "-X", dump]
    if H is not None:
        s += ["--ref-stats-min-hic-ureads-qcov", H]
        t += ["-H", H]
    if p is not None:
        s += ["--ref-stats-min-chunks-fraction", p]
        t += ["-p", p]
    return s, t


def test_the_sample_is_not_one_sided(family):
    """from the ORACLE's TSV, by the restatement: every configuration judges at least 40 references and none of them says one thing only;
    the first one says everything stage 1 can say, each verdict for at least 5 references"""
    text = "\n".join(family["oracle_rows"]) + "\n"
    for i, (tag, level, mode, H, p) in enumerate(CONFIGS):
        v = list(RR.verdicts_of(restated(family, text, tag, level, mode, H, p)).values())
        print(f"taxonomy {tag} level {level} mode {mode} H {H} p {p}: " + ", ".join(f"{x} {v.count(x)}" for x in sorted(VERDICTS)))
        assert len(v) >= 40 and len(set(v)) >= 2 and max(v.count(x) for x in VERDICTS) <= 0.7 * len(v), (tag, mode, v)
        if i == 0:
            assert min(v.count(x) for x in VERDICTS) >= 5, v


def test_cli_equals_kmcp_refstats_and_the_restatement(family, tmp_path):
    plain = str(tmp_path / "plain.tsv")
    run([CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", plain, "-q"])
    text = open(plain).read()
    assert text.startswith(HEADER + "\n") and text.count("\n") > 1500
    seen = set()
    for i, (tag, level, mode, H, p) in enumerate(CONFIGS):
        s, t = flags(family, tag, level, mode, H, p)
        out, stats = str(tmp_path / f"o{i}.tsv"), str(tmp_path / f"s{i}.tsv")
        run([CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", out, "-q", "--ref-stats", stats] + s)
        assert open(out).read() == text, "the search result is what it is without --ref-stats"
        got = open(stats).read()
        assert got == run([TOOL] + t + [plain]).stdout, (tag, level, mode)
        assert got == restated(family, text, tag, level, mode, H, p), (tag, level, mode)
        seen |= set(RR.verdicts_of(got).values())
    assert seen == VERDICTS
    # the level defaults to species where there is a taxonomy, and to strain where there is none; .gz is honoured
    import gzip
    dump, tmap = family["tax"]["B"]
    stats = str(tmp_path / "dstats.tsv.gz")
    run([CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", str(tmp_path / "d.tsv"), "-q", "--ref-stats", stats, "--taxid-map", tmap, "--taxdump", dump])
    assert gzip.open(stats, "rt").read() == restated(family, text, "B", "species", 3, None, None)
    run([CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", str(tmp_path / "d.tsv"), "-q", "--ref-stats", stats[:-3]])
    assert open(stats[:-3]).read() == restated(family, text, None, "strain", 3, None, None)


def test_cli_in_several_batches_with_threads_and_with_the_specific_stage(family, tmp_path):
    tag, level, mode, H, p = CONFIGS[0]
    s, t = flags(family, tag, level, mode, H, p)
    dump, tmap = family["tax"][tag]
    plain = str(tmp_path / "plain.tsv")
    run([CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", plain, "-q"])
    want = run([TOOL] + t + [plain]).stdout
    # 800 reads in batches of 300, four threads
    out, stats = str(tmp_path / "o.tsv"), str(tmp_path / "s.tsv")
    run([CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", out, "-q", "-j", "4", "--gpu-batch", "300", "--ref-stats", stats] + s)
    assert open(stats).read() == want and open(out).read() == open(plain).read()
    # --specific-level beside it: the TSV is the filtered one, the statistics are those of the unfiltered run
    filtered = str(tmp_path / "f.tsv")
    run([CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", filtered, "-q", "--specific-level", "species", "--taxid-map", tmap, "--taxdump", dump])
    run([CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", out, "-q", "--gpu-batch", "300", "--specific-level", "species", "--ref-stats", stats] + s)
    assert open(stats).read() == want
    assert open(out).read() == open(filtered).read() and 50 < open(filtered).read().count("\n") < open(plain).read().count("\n") - 50
    # every read to the host half, and no K3 at all: the same file
    for knob in ("KMCPG_REFSTATS_DEVICE", "KMCPG_DEVICE_FINALIZE"):
        run([CLI, "-d", family["root"], "-t", MIN_QCOV, family["fq"], "-o", out, "-q", "--ref-stats", stats] + s, env=dict(os.environ, **{knob: "0"}))
        assert open(stats).read() == want, knob


# ---- the library ----
def tables(db, family, tag):
    n = int(db.info.n_cols)
    names = [db.col_info(c)[0] for c in range(n)]
    ids = {}
    target = np.array([ids.setdefault(x, len(ids)) for x in names], dtype=np.uint32)
    if tag is None:
        return names, target, None
    dump, tmap = family["tax"][tag]
    taxo, tmap_ids = FR.Taxonomy(dump), FR.read_taxid_maps([tmap])
    return names, target, np.array([next((x for x in taxo.lineage(tmap_ids[n]) if taxo.rank[x] == "species"), 0) for n in names], dtype=np.uint32)


def expected(db, res, level, H, taxid_map=None, tax=None):
    """the restatement on the rows of a library result -> (counters [n_cols, 4], matched, unique)"""
    n = int(db.info.n_cols)
    info = [db.col_info(c) for c in range(n)]
    lines = []
    for r in range(len(res.offs) - 1):
        for m in res.read(r):
            name, tidx, gsize, _ = info[int(m["col"])]
            lines.append("\t".join([f"q{r}", str(res.qlen[r]), str(res.qkmers[r]), "0", "1", name, str(tidx & 0xffff), str(tidx >> 16), str(gsize), "21",
                                    str(int(m["mkmers"])), "%.4f" % (int(m["mkmers"]) / int(res.qkmers[r])), "0", "0", str(r)]))
    prof, matched, unique = RR.stage1(["\n".join(lines)], max_fpr=1, min_qcov=0, hic_min_qcov=H, level=level, taxid_map=taxid_map, tax=tax)
    col_of = {(info[c][0], info[c][1] & 0xffff): c for c in range(n)}
    want = np.zeros((n, 4), dtype=np.uint64)
    for name, t in prof.items():
        for j, l in enumerate((t.rows, t.firsts, t.uniq, t.uniq_hic)):
            for chunk, v in enumerate(l):
                if v:
                    want[col_of[(name, chunk)], j] = int(v)
    return want, matched, unique


def test_library_counts_what_the_restatement_counts_and_changes_no_result(family):
    from kmcp_amd import Database, default_params
    reads = family["reads"] + [family["long_query"]]  # ... and one query above the device's -f bound: the host half counts it
    dump, tmap = family["tax"]["B"]
    tmap_ids, taxo = FR.read_taxid_maps([tmap]), FR.Taxonomy(dump)
    p = default_params(min_qcov=MIN_QCOV)
    with Database.open(family["db_dir"], device=0) as db:
        n = int(db.info.n_cols)
        names, target, species = tables(db, family, "B")
        plain, plain_p = db.search(reads, params=p), db.search_pairs(reads, params=p)
        assert plain.qkmers[-1] > 512 and len(plain.read(len(reads) - 1)) > 0
        want, matched, unique = expected(db, plain, "species", 0.8, tmap_ids, taxo)
        assert matched > 500 and 0.1 * matched < unique < 0.9 * matched
        db.set_refstats(target, species, hic_min_qcov=0.8)
        for form in ("records", "pairs", "tickets", "with K4"):
            db.refstats_reset()
            if form == "records":
                res = db.search(reads, params=p)
                assert all(np.array_equal(getattr(res, f), getattr(plain, f)) for f in ("qlen", "qkmers", "offs", "matches")), "the result changed"
            elif form == "pairs":
                res = db.search_pairs(reads, params=p)
                assert all(np.array_equal(getattr(res, f), getattr(plain_p, f)) for f in ("qlen", "qkmers", "offs", "pairs")), "the result changed"
            elif form == "tickets":  # three batches in flight
                from kmcp_amd import lib
                cuts = [0, 300, 600, len(reads)]
                tickets = [db.submit(*lib.pack_reads(reads[a:b]), params=p) for a, b in zip(cuts, cuts[1:])]
                parts = [db.wait(t) for t in tickets]
                assert sum(len(x.matches) for x in parts) == len(plain.matches)
            else:
                db.set_specific(target, species)
                res = db.search(reads, params=p)
                db.set_specific()
                assert 0 < len(res.matches) < len(plain.matches)
            got, tot = db.refstats_read(n)
            g = got.view(np.uint64).reshape(n, 4)
            bad = np.argwhere(g != want)
            assert len(bad) == 0, f"{form}: column {bad[0][0]}: {g[bad[0][0]]}, expected {want[bad[0][0]]}; {len(bad)} differ"
            assert (tot["matched_reads"], tot["unique_reads"]) == (matched, unique) and tot["host_reads"] >= 1, (form, tot)
        st, _ = db.last_refstats()
        assert st["bad_segments"] == 0 and st["skipped"] == 0
        # what the stage refuses while it is on
        from kmcp_amd.lib import KmcpGpuError
        for kw in (dict(try_se=1), dict(top_n_scores=1)):
            with pytest.raises(KmcpGpuError, match="kmcpg_set_refstats"):
                db.search(reads[:10], params=default_params(**kw))
        seqs, offs = np.frombuffer(family["long_query"], dtype=np.uint8).copy(), np.array([0, 3000], dtype=np.uint64)
        with pytest.raises(KmcpGpuError, match="kmcpg_set_refstats"):
            db.submit_windows(seqs, offs, 100, 300)
        db.set_refstats()
        again = db.search(reads, params=p)
        assert np.array_equal(again.matches, plain.matches)


def test_a_batch_that_is_run_again_is_counted_once(oracle_lib, tmp_path):
    """40 close relatives: every read matches ~35 columns, more than the 8 per read a fresh lane has room for — the first attempt of every
    batch overflows its hit buffer and collect() runs it again (KMCPG_HIT_BUDGET_MB=0: the buffers never grow).  The witness is the
    handle's count of K6 launches that left the counting to a rerun (kmcpg_refstats_totals.skipped_launches), which the command reports.
    (The family sample cannot overflow a hit buffer: it has 2.4 hits per read at -t 0.75 and the plain buffer holds 8 per read.)"""
    from kmcp_amd import Database, default_params
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
    with Database.open(db_dir, device=0) as db:
        n = int(db.info.n_cols)
        names = [db.col_info(c)[0] for c in range(n)]
        ids = {}
        target = np.array([ids.setdefault(x, len(ids)) for x in names], dtype=np.uint32)
        db.set_refstats(target, None, hic_min_qcov=0.75)
        res = db.search(reads, params=default_params())
        assert len(res.matches) > 8 * len(reads) + 1024, "more matches than the first attempt's hit buffer holds"
        want, matched, unique = expected(db, res, "strain", 0.75)
        got, tot = db.refstats_read(n)
        assert np.array_equal(got.view(np.uint64).reshape(n, 4), want) and (tot["matched_reads"], tot["unique_reads"]) == (matched, unique)
        assert matched > 1000 and tot["skipped_launches"] == 1, tot
        # ... and with K4 behind K3 as well: nothing is specific at strain level here, the statistics are the same
        db.refstats_reset()
        db.set_specific(target, None)
        kept = db.search(reads, params=default_params())
        db.set_specific()
        assert len(kept.matches) == 0
        got, tot = db.refstats_read(n)
        assert np.array_equal(got.view(np.uint64).reshape(n, 4), want) and (tot["matched_reads"], tot["unique_reads"]) == (matched, unique)
    # the command, every batch of 400 overflowing: the file kmcp-refstats writes from the TSV
    fq = str(tmp_path / "r.fq")
    with open(fq, "wb") as fh:
        for i, r in enumerate(reads):
            fh.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    out, stats = str(tmp_path / "o.tsv"), str(tmp_path / "s.tsv")
    import re
    r = run([CLI, "-d", os.path.dirname(db_dir), fq, "-o", out, "--gpu-batch", "400", "--ref-stats", stats], env=dict(os.environ, KMCPG_HIT_BUDGET_MB="0"))
    want = run([TOOL, "-f", "1", "-t", "0", "--level", "strain", out]).stdout
    assert open(stats).read() == want and want.count("\n") == 3 + 40
    reruns = re.search(r"\((\d+) batches counted by their rerun", r.stderr)
    assert reruns and int(reruns.group(1)) == 4, r.stderr  # 1500 reads in batches of 400: every one of the four
    # --specific-level beside it: an empty result, the same statistics
    r = run([CLI, "-d", os.path.dirname(db_dir), fq, "-o", str(tmp_path / "f.tsv"), "--gpu-batch", "400", "--ref-stats", stats, "--specific-level", "strain"],
            env=dict(os.environ, KMCPG_HIT_BUDGET_MB="0"))
    assert open(stats).read() == want and int(re.search(r"\((\d+) batches counted by their rerun", r.stderr).group(1)) == 4
    assert not [l for l in open(tmp_path / "f.tsv") if l[0] != "#"]


def test_a_lane_that_counted_serves_a_summary_ticket_next(family):
    """a lane keeps its buffers from batch to batch: after a counted batch, with the stage off again, the same lane takes a batch of window
    summaries (K5) — larger than the counted one — and nothing of the statistics' host half runs on it"""
    from kmcp_amd import Database, default_params
    p = default_params(min_qcov=MIN_QCOV)
    seqs, offs = np.frombuffer(family["long_query"], dtype=np.uint8).copy(), np.array([0, len(family["long_query"])], dtype=np.uint64)
    with Database.open(family["db_dir"], device=0) as db:
        n = int(db.info.n_cols)
        names, target, species = tables(db, family, "B")
        db.set_specific(target, species)
        want = db.wait_summaries(db.submit_windows_summary(seqs, offs, 10, 600, params=p))
        db.set_specific()
        db.set_refstats(target, species, hic_min_qcov=0.8)
        db.search([family["long_query"]] * 3, params=p)  # 3 reads, every one LEFT to the host half
        _, tot = db.refstats_read(n)
        assert tot["host_reads"] == 3
        db.set_refstats()
        db.set_specific(target, species)
        got = db.wait_summaries(db.submit_windows_summary(seqs, offs, 10, 600, params=p))
        assert len(got[0]) > 200 and all(np.array_equal(a, b) for a, b in zip(got, want))
        # ... and with the stage still on, the summary submit is refused and the lane stays usable
        db.set_refstats(target, species, hic_min_qcov=0.8)
        from kmcp_amd.lib import KmcpGpuError
        with pytest.raises(KmcpGpuError, match="kmcpg_set_refstats"):
            db.submit_windows_summary(seqs, offs, 10, 600, params=p)
        db.set_specific()
        db.search([family["long_query"]] * 2, params=p)
        assert db.refstats_read(n)[1]["host_reads"] == 2
